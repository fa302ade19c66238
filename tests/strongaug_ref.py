"""numpy restatement of ``strong_augment`` (DACS's colour jitter and Gaussian blur), the specification the
HIP kernel matches bit for bit (tests/test_strongaug_gpu.py).

Every step is one IEEE operation of ``dtype`` (+ - * / floor, a compare or a select), in the order
written: in float32 this is the specification, in float64 it is the same arithmetic at a precision
where it can be compared with ``colorsys`` and ``scipy.ndimage`` (tests/test_strongaug_cpu.py).
max, min and the clamp are written as compare + select, so that a signed zero or a tie has one
defined result; inputs are finite.

Per image i of a float32 [N, 3, H, W] batch (BGR minus ``mean``):

* jitter (``jitter[i]``):  u_c = (x_c + mean_c) / 255;  r, g, b = u[2], u[1], u[0];  the four ops in
  the order ``order[i]`` (codes ``BRIGHTNESS, CONTRAST, SATURATION, HUE``);  y_c = u_c * 255 - mean_c.
* blur (``radius[i]`` = R > 0), horizontal then vertical, borders reflected without repeating the
  edge:  acc = w[0] x[0];  for d = 1..R: acc = acc + w[d] (x[-d] + x[+d]).
* neither: the input's bits.

Totality of the hue arithmetic: ``h`` is a float in [0, 1] *including 1* (``h6 + 6`` can round to 6
for a tiny negative ``h6``, and ``h - floor(h)`` to 1 for a tiny negative ``h``).  ``hsv_to_rgb`` takes
``i = floor(6 h)``, ``f = 6 h - i`` and, when ``i >= 6`` (only at h == 1, where f == 0), uses sector 0:
h == 1 is the colour of h == 0.
"""
import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
MAX_RADIUS = 7
IMG_MEAN = np.array((104.00698793, 116.66876762, 122.67891434), dtype=np.float32)

# what the last jitter() call went through, for the tests' coverage assertions
STATS: dict = {}


def _count(key, mask):
    STATS[key] = STATS.get(key, 0) + int(np.count_nonzero(mask))


def _max(a, b):
    return np.where(a > b, a, b)


def _min(a, b):
    return np.where(a < b, a, b)


def clamp01(x, key=None):
    t = x.dtype.type
    if key is not None:
        _count(key + "_lo", x < 0)
        _count(key + "_hi", x > 1)
    return np.where(x < 0, t(0), np.where(x > 1, t(1), x))


def rgb_to_hsv(r, g, b):
    t = r.dtype.type
    mx = _max(_max(r, g), b)
    mn = _min(_min(r, g), b)
    d = mx - mn
    safe_mx = np.where(mx > 0, mx, t(1))
    s = np.where(mx > 0, d / safe_mx, t(0))
    dd = np.where(d == 0, t(1), d)
    is_r, is_g = mx == r, mx == g
    h6 = np.where(d == 0, t(0),
                  np.where(is_r, (g - b) / dd, np.where(is_g, t(2) + (b - r) / dd, t(4) + (r - g) / dd)))
    _count("grey", d == 0)
    _count("black", ~(mx > 0))
    _count("max_r", (d != 0) & is_r)
    _count("max_g", (d != 0) & ~is_r & is_g)
    _count("max_b", (d != 0) & ~is_r & ~is_g)
    h6 = np.where(h6 < 0, h6 + t(6), h6)
    return h6 / t(6), s, mx


def hsv_to_rgb(h, s, v):
    t = h.dtype.type
    h6 = h * t(6)
    i = np.floor(h6)
    f = h6 - i
    i = np.where(i >= 6, t(0), i)   # h == 1 (f == 0): the colour of h == 0
    p = v * (t(1) - s)
    q = v * (t(1) - s * f)
    u = v * (t(1) - s * (t(1) - f))
    r = np.where(i == 0, v, np.where(i == 1, q, np.where(i == 2, p, np.where(i == 3, p, np.where(i == 4, u, v)))))
    g = np.where(i == 0, u, np.where(i == 1, v, np.where(i == 2, v, np.where(i == 3, q, p))))
    b = np.where(i == 0, p, np.where(i == 1, p, np.where(i == 2, u, np.where(i == 3, v, np.where(i == 4, v, q)))))
    return r, g, b


def op_brightness(r, g, b, db):
    return tuple(clamp01(c + db, "bright") for c in (r, g, b))


def op_contrast(r, g, b, fc):
    return tuple(clamp01(c * fc, "contrast") for c in (r, g, b))


def op_saturation(r, g, b, fs):
    h, s, v = rgb_to_hsv(r, g, b)
    return hsv_to_rgb(h, clamp01(s * fs), v)


def op_hue(r, g, b, fh):
    h, s, v = rgb_to_hsv(r, g, b)
    h = h + fh
    fl = np.floor(h)
    _count("wrap_down", fl > 0)   # h + fh >= 1
    _count("wrap_up", fl < 0)     # h + fh < 0
    return hsv_to_rgb(h - fl, s, v)


OPS = {BRIGHTNESS: op_brightness, CONTRAST: op_contrast, SATURATION: op_saturation, HUE: op_hue}


def jitter(x, mean, db, fc, fs, fh, order, dtype=np.float32):
    """x [3, H, W] (BGR minus mean) -> the jittered image, same layout."""
    t = np.dtype(dtype).type
    x = x.astype(dtype)
    mean = np.asarray(mean).astype(dtype)
    u = [(x[c] + mean[c]) / t(255) for c in range(3)]
    r, g, b = u[2], u[1], u[0]
    fac = {BRIGHTNESS: t(db), CONTRAST: t(fc), SATURATION: t(fs), HUE: t(fh)}
    for code in order:
        r, g, b = OPS[int(code)](r, g, b, fac[int(code)])
    return np.stack([c * t(255) - mean[k] for k, c in enumerate((b, g, r))])


def reflect(i, n):
    """Index i in [-(n - 1), 2 (n - 1)] reflected into [0, n) without repeating the edge (-1 -> 1)."""
    i = np.where(i < 0, -i, i)
    return np.where(i > n - 1, 2 * (n - 1) - i, i)


def blur_axis(x, w, radius, axis):
    """One pass along ``axis`` of x [..]: acc = w[0] x[0]; acc = acc + w[d] (x[-d] + x[+d]), d ascending."""
    n = x.shape[axis]
    if radius > n - 1:
        raise ValueError(f"blur radius {radius} on an axis of {n} (expected R <= n - 1)")
    idx = np.arange(n)
    acc = w[0] * x
    for d in range(1, int(radius) + 1):
        lo = np.take(x, reflect(idx - d, n), axis=axis)
        hi = np.take(x, reflect(idx + d, n), axis=axis)
        acc = acc + w[d] * (lo + hi)
    return acc


def blur(x, w, radius, dtype=np.float32):
    """x [3, H, W]; w: the half kernel [8]; horizontal first, then vertical."""
    x = x.astype(dtype)
    w = np.asarray(w).astype(dtype)
    return blur_axis(blur_axis(x, w, radius, 2), w, radius, 1)


def strong_augment(images, params, mean=IMG_MEAN, dtype=np.float32):
    """images float32 [N, 3, H, W]; params: ``StrongAugSampler.sample``'s dictionary."""
    STATS.clear()
    out = []
    for i in range(images.shape[0]):
        x = images[i]
        on, rad = bool(params["jitter"][i]), int(params["radius"][i])
        if not on and rad == 0:
            out.append(x.astype(dtype, copy=True))   # the input's bits
            continue
        if on:
            x = jitter(x, mean, params["db"][i], params["fc"][i], params["fs"][i], params["fh"][i],
                       params["order"][i], dtype)
        if rad > 0:
            x = blur(x, params["weights"][i], rad, dtype)
        out.append(x.astype(dtype))
    return np.stack(out)
