// GTA5 / Cityscapes input pipeline on the GPU: the arithmetic of
// GTA5DataSet.__getitem__ (reference dataset/gta5_dataset.py:47-71) after file decode,
//   image.resize(crop, BICUBIC); label.resize(crop, NEAREST); id -> trainId (255 elsewhere);
//   RGB -> BGR; -= IMG_MEAN (float32); HWC -> CHW
// reproduced bit-exactly.  The resize is Pillow's 8-bpc separable resampler (the library the
// reference calls): per output pixel a window [xmin, xmin+n) and n weights of the bicubic
// kernel (a = -0.5) stretched by the downscale factor, normalised in double and rounded to
// 22-bit fixed point; a horizontal pass then a vertical pass, each accumulating in int32 from
// 2^21 and clamping (acc >> 22) to uint8.  NEAREST takes floor((x + 0.5) * scale) with the
// coordinate accumulated in double, as Pillow's affine transform does.
//
// Kernels: resize_coeff_kernel builds the weight tables on the device in double with FP
// contraction off (so they equal the host's / Pillow's); resize_h_kernel (uint8 RGB ->
// uint8 [n][in_h][out_w][3]); resize_v_bgr_kernel (-> float NCHW BGR - mean); label_kernel.
// All byte/integer work, HBM-bound: one read of the source image and labels, one write of
// the float image and int64 labels (plus the out_w-wide uint8 intermediate).
// The augment_* kernels further down are the same pipeline with a per-sample scale, crop / pad
// window and horizontal mirror (adaptseg_gta5_preprocess_augment).
#include "common.hpp"
#include <algorithm>
#include <cmath>

namespace adaptseg {

constexpr int kPrecisionBits = 32 - 8 - 2;
constexpr int kMaxKsize = 64;  // ceil(2 * downscale) * 2 + 1 <= 64: downscale up to 15x

#pragma clang fp contract(off)
__device__ double bicubic_filter(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

struct ResizeTables {
  int ksx, ksy;        // taps per output pixel (x, y)
  int *bx, *by;        // [out][2] = (first source index, count)
  int *kx, *ky;        // [out][ks] fixed-point weights
  int *nx, *ny;        // nearest source index per output column / row
};

// Window and weights of output pixel `o`: bounds[2] = (first source index, count), kk[ks].
__device__ void coeffs_at(int in_size, int out_size, int o, int ks, int *bounds, int *kk) {
  const double scale = (double)in_size / (double)out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * filterscale;
  const double ss = 1.0 / filterscale;
  const double center = ((double)o + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  // two passes over the (deterministic) filter instead of a per-thread weight array, which
  // would live in scratch: the sum first, then each normalised weight
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += bicubic_filter(((double)(x + xmin) - center + 0.5) * ss);
  for (int x = 0; x < ks; ++x) {
    const double w = x < xmax ? bicubic_filter(((double)(x + xmin) - center + 0.5) * ss) : 0.0;
    const double v = ww != 0.0 ? w / ww : w;
    kk[x] = v < 0 ? (int)(-0.5 + v * (double)(1 << kPrecisionBits))
                                   : (int)(0.5 + v * (double)(1 << kPrecisionBits));
  }
  bounds[0] = xmin;
  bounds[1] = xmax;
}

__device__ void coeffs_one(int in_size, int out_size, int o, int ks, int *bounds, int *kk) {
  coeffs_at(in_size, out_size, o, ks, bounds + 2 * o, kk + (size_t)o * ks);
}

// threads [0, out_w) -> x weights, [out_w, out_w + out_h) -> y weights; the last two
// threads walk the NEAREST coordinates (a sequential double accumulation, as Pillow).
__global__ void resize_coeff_kernel(int in_h, int in_w, int out_h, int out_w, ResizeTables t) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < out_w) coeffs_one(in_w, out_w, i, t.ksx, t.bx, t.kx);
  else if (i < out_w + out_h) coeffs_one(in_h, out_h, i - out_w, t.ksy, t.by, t.ky);
  else if (i == out_w + out_h || i == out_w + out_h + 1) {
    const bool xs = i == out_w + out_h;
    const int in = xs ? in_w : in_h, out = xs ? out_w : out_h;
    int *dst = xs ? t.nx : t.ny;
    const double scale = (double)in / (double)out;
    double v = 0.5 * scale;
    for (int o = 0; o < out; ++o) {
      const int s = (int)v;
      dst[o] = s < in - 1 ? s : in - 1;
      v += scale;
    }
  }
}
#pragma clang fp contract(on)

__device__ __forceinline__ unsigned clip8(int acc) {
  const int v = acc >> kPrecisionBits;
  return (unsigned)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// Horizontal pass: src [n][in_h][in_w][3] -> tmp [n][in_h][out_w][3] (uint8, Pillow-rounded).
__global__ void resize_h_kernel(int n, int in_h, int in_w, int out_w, const uint8_t *__restrict__ src,
                                ResizeTables t, uint8_t *__restrict__ tmp) {
  const int64_t total = (int64_t)n * in_h * out_w;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xo = (int)(i % out_w);
    const int64_t row = i / out_w;  // n * in_h + y
    const int x0 = t.bx[2 * xo], cnt = t.bx[2 * xo + 1];
    const int *k = t.kx + (size_t)xo * t.ksx;
    const uint8_t *s = src + (row * in_w + x0) * 3;
    int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < cnt; ++j) {
      const int w = k[j];
      a0 += s[3 * j] * w;
      a1 += s[3 * j + 1] * w;
      a2 += s[3 * j + 2] * w;
    }
    uint8_t *d = tmp + i * 3;
    d[0] = (uint8_t)clip8(a0);
    d[1] = (uint8_t)clip8(a1);
    d[2] = (uint8_t)clip8(a2);
  }
}

// Vertical pass + BGR + mean + CHW: tmp [n][in_h][out_w][3] -> out [n][3][out_h][out_w] with
// out[c'] = float(rgb[2 - c']) - mean[c'] (float32, as image -= IMG_MEAN).
__global__ void resize_v_bgr_kernel(int n, int in_h, int out_h, int out_w, const uint8_t *__restrict__ tmp,
                                    ResizeTables t, float m0, float m1, float m2, float *__restrict__ out) {
  const int64_t total = (int64_t)n * out_h * out_w;
  const int64_t plane = (int64_t)out_h * out_w;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xo = (int)(i % out_w);
    const int64_t r = i / out_w;
    const int yo = (int)(r % out_h);
    const int b = (int)(r / out_h);
    const int y0 = t.by[2 * yo], cnt = t.by[2 * yo + 1];
    const int *k = t.ky + (size_t)yo * t.ksy;
    const uint8_t *s = tmp + (((int64_t)b * in_h + y0) * out_w + xo) * 3;
    const int64_t stride = (int64_t)out_w * 3;
    int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < cnt; ++j) {
      const int w = k[j];
      a0 += s[j * stride] * w;
      a1 += s[j * stride + 1] * w;
      a2 += s[j * stride + 2] * w;
    }
    float *o = out + (int64_t)b * 3 * plane + (int64_t)yo * out_w + xo;
    o[0] = (float)clip8(a2) - m0;  // B
    o[plane] = (float)clip8(a1) - m1;  // G
    o[2 * plane] = (float)clip8(a0) - m2;  // R
  }
}

// labels [n][in_h][in_w] uint8 ids -> [n][out_h][out_w] int64 trainIds (lut[256], int32).
__global__ void label_kernel(int n, int in_h, int in_w, int out_h, int out_w, const uint8_t *__restrict__ ids,
                             ResizeTables t, const int32_t *__restrict__ lut, int64_t *__restrict__ out) {
  const int64_t total = (int64_t)n * out_h * out_w;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xo = (int)(i % out_w);
    const int64_t r = i / out_w;
    const int yo = (int)(r % out_h);
    const int b = (int)(r / out_h);
    const uint8_t id = ids[((int64_t)b * in_h + t.ny[yo]) * in_w + t.nx[xo]];
    out[i] = lut ? (int64_t)lut[id] : (int64_t)id;
  }
}

// ---- random scale / crop / mirror (adaptseg_gta5_preprocess_augment) ---------------------------
// Sample b is resized to its own (sw, sh), flipped left-right if `mirror`, and the crop window
// [ox, ox + cw) x [oy, oy + ch) of that image is written; outside it the image is 0.0f and the
// label ignore_label.  The tables are per sample and per window position, so the scaled image
// is never materialised: window column x reads column xc = mirror ? sw-1-(x+ox) : x+ox of the
// resize, window row y reads row y+oy.  A position outside the scaled image has count 0 in
// bx / by and -1 in nx / ny; the vertical and label kernels write the padding from that.
// The horizontal pass keeps, per sample, only the source rows [r0, r0 + nrows) that the
// window's rows read (computed on the host, which also sizes the workspace from them).
constexpr int kAugChunk = 16;  // samples per coefficient launch (their parameters are kernel arguments)

struct AugChunk {
  int p[kAugChunk][7];  // sw, sh, ox, oy, mirror, r0, nrows
};

struct AugTables {
  int ksx, ksy;        // taps per output pixel: the batch maximum
  int rmax;            // rows of tmp per sample: the batch maximum of nrows (at least 1)
  int *bx, *by;        // [n][cw][2], [n][ch][2] = (first source index, count); count 0 = padding
  int *kx, *ky;        // [n][cw][ksx], [n][ch][ksy]
  int *nx, *ny;        // [n][cw], [n][ch] nearest source index, -1 = padding
  int *rows;           // [n][2] = (r0, nrows)
};

#pragma clang fp contract(off)
// grid (ceil((cw + ch + 3) / 64), samples of the chunk): threads [0, cw) -> x weights,
// [cw, cw + ch) -> y weights, the next two walk the NEAREST coordinates from 0 (Pillow's
// sequential double accumulation) up to the last column / row the window reads, one more
// stores the sample's source-row range.
__global__ void augment_coeff_kernel(int first, int in_h, int in_w, int ch, int cw, AugChunk c, AugTables t) {
  const int s = blockIdx.y, b = first + s;
  const int sw = c.p[s][0], sh = c.p[s][1], ox = c.p[s][2], oy = c.p[s][3], mirror = c.p[s][4];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cw + ch) {
    const bool xs = i < cw;
    const int w = xs ? i : i - cw;                     // window position
    const int r = w + (xs ? ox : oy);                  // position in the (flipped) scaled image
    const int out = xs ? sw : sh, span = xs ? cw : ch, ks = xs ? t.ksx : t.ksy;
    const size_t e = (size_t)b * span + w;
    int *bounds = (xs ? t.bx : t.by) + 2 * e;
    if (r >= 0 && r < out) {
      coeffs_at(xs ? in_w : in_h, out, xs && mirror ? sw - 1 - r : r, ks, bounds, (xs ? t.kx : t.ky) + e * ks);
    } else {
      bounds[0] = 0;
      bounds[1] = 0;
      (xs ? t.nx : t.ny)[e] = -1;
    }
  } else if (i == cw + ch || i == cw + ch + 1) {
    const bool xs = i == cw + ch;
    const int in = xs ? in_w : in_h, out = xs ? sw : sh, span = xs ? cw : ch, off = xs ? ox : oy;
    const bool flip = xs && mirror;
    // scaled positions [lo, end) are the ones inside the window: position o lands on window
    // position o - off, or out - 1 - o - off when flipped
    const int lo = flip ? (out - off - span > 0 ? out - off - span : 0) : (off > 0 ? off : 0);
    const int end = flip ? (out - off < out ? out - off : out) : (off + span < out ? off + span : out);
    if (lo < end) {
      int *d = (xs ? t.nx : t.ny) + (size_t)b * span + (flip ? out - 1 - lo - off : lo - off);
      const int step = flip ? -1 : 1;
      const double scale = (double)in / (double)out;
      double v = 0.5 * scale;
      int o = 0;
      for (; o < lo; ++o) v += scale;  // the walk is serial: keep the skipped part to one add each
      for (; o < end; ++o) {
        const int sidx = (int)v;
        *d = sidx < in - 1 ? sidx : in - 1;
        d += step;
        v += scale;
      }
    }
  } else if (i == cw + ch + 2) {
    t.rows[2 * b] = c.p[s][5];
    t.rows[2 * b + 1] = c.p[s][6];
  }
}
#pragma clang fp contract(on)

// Horizontal pass over the window: src [n][in_h][in_w][3] -> tmp [n][rmax][cw][3], row rr of
// sample b being source row r0 + rr.  Padding columns and rows past nrows are left unwritten
// (the vertical pass does not read them).
__global__ void augment_h_kernel(int n, int in_h, int in_w, int cw, const uint8_t *__restrict__ src, AugTables t,
                                 uint8_t *__restrict__ tmp) {
  const int64_t total = (int64_t)n * t.rmax * cw;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xo = (int)(i % cw);
    const int64_t r = i / cw;
    const int rr = (int)(r % t.rmax);
    const int b = (int)(r / t.rmax);
    const int64_t e = (int64_t)b * cw + xo;
    const int x0 = t.bx[2 * e], cnt = t.bx[2 * e + 1];
    if (rr >= t.rows[2 * b + 1] || cnt == 0) continue;
    const int *k = t.kx + e * t.ksx;
    const uint8_t *s = src + (((int64_t)b * in_h + t.rows[2 * b] + rr) * in_w + x0) * 3;
    int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < cnt; ++j) {
      const int w = k[j];
      a0 += s[3 * j] * w;
      a1 += s[3 * j + 1] * w;
      a2 += s[3 * j + 2] * w;
    }
    uint8_t *d = tmp + i * 3;
    d[0] = (uint8_t)clip8(a0);
    d[1] = (uint8_t)clip8(a1);
    d[2] = (uint8_t)clip8(a2);
  }
}

// Vertical pass + BGR + mean + CHW over the window, and the image's padding (0.0f: a pixel
// equal to the mean).  The tmp row index is clamped to the sample's slab.
__global__ void augment_v_bgr_kernel(int n, int ch, int cw, const uint8_t *__restrict__ tmp, AugTables t, float m0,
                                     float m1, float m2, float *__restrict__ out) {
  const int64_t total = (int64_t)n * ch * cw;
  const int64_t plane = (int64_t)ch * cw;
  const int64_t stride = (int64_t)cw * 3;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xo = (int)(i % cw);
    const int64_t r = i / cw;
    const int yo = (int)(r % ch);
    const int b = (int)(r / ch);
    const int64_t ey = (int64_t)b * ch + yo;
    const int y0 = t.by[2 * ey] - t.rows[2 * b], cnt = t.by[2 * ey + 1];
    const bool inside = cnt != 0 && t.bx[2 * ((int64_t)b * cw + xo) + 1] != 0;
    float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
    if (inside) {
      const int *k = t.ky + ey * t.ksy;
      const uint8_t *s = tmp + ((int64_t)b * t.rmax * cw + xo) * 3;
      int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
      for (int j = 0; j < cnt; ++j) {
        const int w = k[j];
        int rr = y0 + j;
        rr = rr < 0 ? 0 : rr > t.rmax - 1 ? t.rmax - 1 : rr;
        const uint8_t *p = s + rr * stride;
        a0 += p[0] * w;
        a1 += p[1] * w;
        a2 += p[2] * w;
      }
      v0 = (float)clip8(a2) - m0;  // B
      v1 = (float)clip8(a1) - m1;  // G
      v2 = (float)clip8(a0) - m2;  // R
    }
    float *o = out + (int64_t)b * 3 * plane + (int64_t)yo * cw + xo;
    o[0] = v0;
    o[plane] = v1;
    o[2 * plane] = v2;
  }
}

// labels [n][in_h][in_w] uint8 ids -> the window's [n][ch][cw] int64 trainIds, ignore_label
// outside the scaled image.
__global__ void augment_label_kernel(int n, int in_h, int in_w, int ch, int cw, const uint8_t *__restrict__ ids,
                                     AugTables t, const int32_t *__restrict__ lut, int64_t ignore_label,
                                     int64_t *__restrict__ out) {
  const int64_t total = (int64_t)n * ch * cw;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xo = (int)(i % cw);
    const int64_t r = i / cw;
    const int yo = (int)(r % ch);
    const int b = (int)(r / ch);
    const int sx = t.nx[(int64_t)b * cw + xo], sy = t.ny[(int64_t)b * ch + yo];
    int64_t v = ignore_label;
    if (sx >= 0 && sy >= 0) {
      const uint8_t id = ids[((int64_t)b * in_h + sy) * in_w + sx];
      v = lut ? (int64_t)lut[id] : (int64_t)id;
    }
    out[i] = v;
  }
}

static int ksize_for(int in_size, int out_size) {
  const double scale = (double)in_size / (double)out_size;
  const double support = 2.0 * (scale < 1.0 ? 1.0 : scale);
  return (int)std::ceil(support) * 2 + 1;
}

static size_t a256(size_t b) { return (b + 255) / 256 * 256; }

struct WsLayout {
  size_t bx, kx, by, ky, nx, ny, tmp, total;
};

static WsLayout ws_layout(int n, int in_h, int in_w, int out_h, int out_w) {
  WsLayout l;
  const int ksx = ksize_for(in_w, out_w), ksy = ksize_for(in_h, out_h);
  size_t o = 0;
  l.bx = o; o += a256((size_t)out_w * 2 * 4);
  l.kx = o; o += a256((size_t)out_w * ksx * 4);
  l.by = o; o += a256((size_t)out_h * 2 * 4);
  l.ky = o; o += a256((size_t)out_h * ksy * 4);
  l.nx = o; o += a256((size_t)out_w * 4);
  l.ny = o; o += a256((size_t)out_h * 4);
  l.tmp = o; o += a256((size_t)n * in_h * out_w * 3);
  l.total = o;
  return l;
}

static int grid_for(int64_t total) { return (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(total, 256), 16384)); }

constexpr int kAugMaxOffset = 1 << 20;  // |ox|, |oy|, sw, sh stay below it: window arithmetic fits int32

// Source rows [r0, r0 + nrows) that the window rows inside the scaled image read: the taps of
// its first and last such row (coeffs_at's arithmetic), widened by one row on each side so a
// last-bit difference between host and device rounding cannot matter.
static void aug_rows(int in_h, int sh, int oy, int ch, int *r0, int *nrows) {
  const int ylo = std::max(0, -oy), yhi = std::min(ch, sh - oy);
  *r0 = *nrows = 0;
  if (ylo >= yhi) return;
  const double scale = (double)in_h / (double)sh;
  const double support = 2.0 * (scale < 1.0 ? 1.0 : scale);
  const double lo = std::floor(((double)(ylo + oy) + 0.5) * scale - support + 0.5) - 1.0;
  const double hi = std::floor(((double)(yhi - 1 + oy) + 0.5) * scale + support + 0.5) + 1.0;
  *r0 = (int)std::max(lo, 0.0);
  *nrows = (int)std::min(hi, (double)in_h) - *r0;
}

struct AugLayout {
  int ksx, ksy, rmax;
  size_t bx, kx, by, ky, nx, ny, rows, tmp, total;
};

// Host validation of an augmented call's geometry and parameters, and its workspace layout.
static int aug_plan(int n, int in_h, int in_w, int ch, int cw, const int32_t *params, AugLayout *l) {
  AS_CHECK_ARG(n > 0 && in_h > 0 && in_w > 0 && ch > 0 && cw > 0, "preprocess_augment: bad sizes");
  AS_CHECK_ARG(ch < kAugMaxOffset && cw < kAugMaxOffset, "preprocess_augment: crop size too large");
  AS_CHECK_ARG(params, "preprocess_augment: null params");
  AS_CHECK_ARG((int64_t)n * in_h * in_w * 3 < (1ll << 40), "preprocess_augment: input too large");
  l->ksx = l->ksy = 0;
  l->rmax = 1;
  for (int b = 0; b < n; ++b) {
    const int32_t *p = params + 5 * b;
    AS_CHECK_ARG(p[0] >= 1 && p[1] >= 1 && p[0] < kAugMaxOffset && p[1] < kAugMaxOffset,
                 "preprocess_augment: bad scaled size %d x %d of sample %d", p[0], p[1], b);
    AS_CHECK_ARG(p[2] > -kAugMaxOffset && p[2] < kAugMaxOffset && p[3] > -kAugMaxOffset && p[3] < kAugMaxOffset,
                 "preprocess_augment: bad offset (%d, %d) of sample %d", p[2], p[3], b);
    AS_CHECK_ARG(p[4] == 0 || p[4] == 1, "preprocess_augment: bad mirror flag %d of sample %d", p[4], b);
    const int ksx = ksize_for(in_w, p[0]), ksy = ksize_for(in_h, p[1]);
    AS_CHECK_ARG(ksx <= kMaxKsize && ksy <= kMaxKsize, "preprocess_augment: downscale factor above 15 not supported");
    int r0, nrows;
    aug_rows(in_h, p[1], p[3], ch, &r0, &nrows);
    l->ksx = std::max(l->ksx, ksx);
    l->ksy = std::max(l->ksy, ksy);
    l->rmax = std::max(l->rmax, nrows);
  }
  size_t o = 0;
  l->bx = o; o += a256((size_t)n * cw * 2 * 4);
  l->kx = o; o += a256((size_t)n * cw * l->ksx * 4);
  l->by = o; o += a256((size_t)n * ch * 2 * 4);
  l->ky = o; o += a256((size_t)n * ch * l->ksy * 4);
  l->nx = o; o += a256((size_t)n * cw * 4);
  l->ny = o; o += a256((size_t)n * ch * 4);
  l->rows = o; o += a256((size_t)n * 2 * 4);
  l->tmp = o; o += a256((size_t)n * l->rmax * cw * 3);
  l->total = o;
  return ADAPTSEG_OK;
}

}  // namespace adaptseg

using namespace adaptseg;

extern "C" {

int adaptseg_preprocess_workspace_size(int n, int in_h, int in_w, int out_h, int out_w, size_t *bytes) {
  AS_CHECK_ARG(bytes && n > 0 && in_h > 0 && in_w > 0 && out_h > 0 && out_w > 0, "preprocess_workspace_size: bad args");
  AS_CHECK_ARG(ksize_for(in_w, out_w) <= kMaxKsize && ksize_for(in_h, out_h) <= kMaxKsize,
               "preprocess: downscale factor above 15 not supported");
  *bytes = ws_layout(n, in_h, in_w, out_h, out_w).total;
  return ADAPTSEG_OK;
}

int adaptseg_gta5_preprocess(int n, int in_h, int in_w, int out_h, int out_w, const uint8_t *rgb, float mean_b,
                             float mean_g, float mean_r, float *image, const uint8_t *label_ids, const int32_t *lut,
                             int64_t *labels, void *ws, size_t ws_bytes, adaptseg_stream_t stream) {
  AS_CHECK_ARG(n > 0 && in_h > 0 && in_w > 0 && out_h > 0 && out_w > 0, "gta5_preprocess: bad sizes");
  AS_CHECK_ARG(rgb && image, "gta5_preprocess: null image pointer");
  AS_CHECK_ARG(!label_ids == !labels, "gta5_preprocess: label_ids and labels go together");
  AS_CHECK_ARG((int64_t)n * in_h * in_w * 3 < (1ll << 40), "gta5_preprocess: input too large");
  AS_CHECK_ARG(ksize_for(in_w, out_w) <= kMaxKsize && ksize_for(in_h, out_h) <= kMaxKsize,
               "gta5_preprocess: downscale factor above 15 not supported");
  const WsLayout l = ws_layout(n, in_h, in_w, out_h, out_w);
  if (!ws || ws_bytes < l.total) {
    set_error("gta5_preprocess: workspace %zu < required %zu", ws_bytes, l.total);
    return ADAPTSEG_ERR_WORKSPACE;
  }
  char *base = reinterpret_cast<char *>(ws);
  ResizeTables t;
  t.ksx = ksize_for(in_w, out_w);
  t.ksy = ksize_for(in_h, out_h);
  t.bx = reinterpret_cast<int *>(base + l.bx);
  t.kx = reinterpret_cast<int *>(base + l.kx);
  t.by = reinterpret_cast<int *>(base + l.by);
  t.ky = reinterpret_cast<int *>(base + l.ky);
  t.nx = reinterpret_cast<int *>(base + l.nx);
  t.ny = reinterpret_cast<int *>(base + l.ny);
  uint8_t *tmp = reinterpret_cast<uint8_t *>(base + l.tmp);
  hipStream_t s = as_stream(stream);
  resize_coeff_kernel<<<(unsigned)ceil_div(out_w + out_h + 2, 64), 64, 0, s>>>(in_h, in_w, out_h, out_w, t);
  AS_CHECK_LAUNCH("resize_coeff");
  // Pillow skips a pass whose size is unchanged; the identity table (one tap of 2^22) gives
  // the same bytes, so both passes always run.
  resize_h_kernel<<<grid_for((int64_t)n * in_h * out_w), 256, 0, s>>>(n, in_h, in_w, out_w, rgb, t, tmp);
  AS_CHECK_LAUNCH("resize_h");
  resize_v_bgr_kernel<<<grid_for((int64_t)n * out_h * out_w), 256, 0, s>>>(n, in_h, out_h, out_w, tmp, t, mean_b,
                                                                           mean_g, mean_r, image);
  AS_CHECK_LAUNCH("resize_v_bgr");
  if (label_ids) {
    label_kernel<<<grid_for((int64_t)n * out_h * out_w), 256, 0, s>>>(n, in_h, in_w, out_h, out_w, label_ids, t,
                                                                      lut, labels);
    AS_CHECK_LAUNCH("label");
  }
  return ADAPTSEG_OK;
}

int adaptseg_preprocess_augment_workspace_size(int n, int in_h, int in_w, int out_h, int out_w, const int32_t *params,
                                               size_t *bytes) {
  AS_CHECK_ARG(bytes, "preprocess_augment_workspace_size: null bytes");
  AugLayout l;
  const int st = aug_plan(n, in_h, in_w, out_h, out_w, params, &l);
  if (st != ADAPTSEG_OK) return st;
  *bytes = l.total;
  return ADAPTSEG_OK;
}

int adaptseg_gta5_preprocess_augment(int n, int in_h, int in_w, int out_h, int out_w, const uint8_t *rgb,
                                     float mean_b, float mean_g, float mean_r, float *image,
                                     const uint8_t *label_ids, const int32_t *lut, int64_t *labels,
                                     const int32_t *params, int ignore_label, void *ws, size_t ws_bytes,
                                     adaptseg_stream_t stream) {
  AugLayout l;
  const int st = aug_plan(n, in_h, in_w, out_h, out_w, params, &l);
  if (st != ADAPTSEG_OK) return st;
  AS_CHECK_ARG(rgb && image, "gta5_preprocess_augment: null image pointer");
  AS_CHECK_ARG(!label_ids == !labels, "gta5_preprocess_augment: label_ids and labels go together");
  if (!ws || ws_bytes < l.total) {
    set_error("gta5_preprocess_augment: workspace %zu < required %zu", ws_bytes, l.total);
    return ADAPTSEG_ERR_WORKSPACE;
  }
  char *base = reinterpret_cast<char *>(ws);
  AugTables t;
  t.ksx = l.ksx;
  t.ksy = l.ksy;
  t.rmax = l.rmax;
  t.bx = reinterpret_cast<int *>(base + l.bx);
  t.kx = reinterpret_cast<int *>(base + l.kx);
  t.by = reinterpret_cast<int *>(base + l.by);
  t.ky = reinterpret_cast<int *>(base + l.ky);
  t.nx = reinterpret_cast<int *>(base + l.nx);
  t.ny = reinterpret_cast<int *>(base + l.ny);
  t.rows = reinterpret_cast<int *>(base + l.rows);
  uint8_t *tmp = reinterpret_cast<uint8_t *>(base + l.tmp);
  hipStream_t s = as_stream(stream);
  for (int first = 0; first < n; first += kAugChunk) {
    const int m = std::min(kAugChunk, n - first);
    AugChunk c = {};
    for (int i = 0; i < m; ++i) {
      const int32_t *p = params + 5 * (first + i);
      for (int j = 0; j < 5; ++j) c.p[i][j] = p[j];
      aug_rows(in_h, p[1], p[3], out_h, &c.p[i][5], &c.p[i][6]);
    }
    augment_coeff_kernel<<<dim3((unsigned)ceil_div(out_w + out_h + 3, 64), (unsigned)m), 64, 0, s>>>(
        first, in_h, in_w, out_h, out_w, c, t);
    AS_CHECK_LAUNCH("augment_coeff");
  }
  augment_h_kernel<<<grid_for((int64_t)n * l.rmax * out_w), 256, 0, s>>>(n, in_h, in_w, out_w, rgb, t, tmp);
  AS_CHECK_LAUNCH("augment_h");
  augment_v_bgr_kernel<<<grid_for((int64_t)n * out_h * out_w), 256, 0, s>>>(n, out_h, out_w, tmp, t, mean_b, mean_g,
                                                                            mean_r, image);
  AS_CHECK_LAUNCH("augment_v_bgr");
  if (label_ids) {
    augment_label_kernel<<<grid_for((int64_t)n * out_h * out_w), 256, 0, s>>>(n, in_h, in_w, out_h, out_w, label_ids,
                                                                              t, lut, (int64_t)ignore_label, labels);
    AS_CHECK_LAUNCH("augment_label");
  }
  return ADAPTSEG_OK;
}

}  // extern "C"
