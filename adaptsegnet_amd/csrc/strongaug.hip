// DACS's "strong" transform of ClassMix's mixed images: a colour jitter, then a Gaussian blur,
// each per image and optional, in ONE launch for the whole batch.
//   strong_augment   grid (tiles, images); the block branches on its image's (block-uniform) controls:
//                    R == 0: per-pixel path (copy, or jitter) over the 1024 pixels of index blockIdx.x
//                    R  > 0: tile path: tile + halo of the three planes staged in LDS, jittered once per
//                            staged pixel on the way in; horizontal pass into a second LDS plane
//                            (vertical halo rows included); vertical pass LDS -> registers -> stores
// tests/strongaug_ref.py restates the arithmetic in numpy; the kernel matches it bit for bit: every
// step is one fp32 + - * / floor, a compare or a select, nothing contracts, '/' is correctly rounded.
//
// Tile: 64 x 16 outputs, 256 threads.  With the largest halo (7) the staged planes are
// 3 x 30 x 78 x 4 B = 28080 B and the horizontal plane (one channel at a time) 30 x 64 x 4 B =
// 7680 B: 35760 B per block, four blocks (16 waves) per CU under the 160 KiB of LDS.  A taller or
// wider tile lowers the halo's read amplification (2.3 x at R = 7, served by L2) but drops a CU to
// two or three blocks; rows of 64 floats keep every LDS access of a wave on 64 consecutive words
// (conflict free) and every global store of a wave one 256-byte row segment.
#include "common.hpp"

#pragma clang fp contract(off)   // the restatement rounds every product and sum on its own

namespace adaptseg {

namespace {

constexpr int kAugThreads = 256;
constexpr int kTileW = 64, kTileH = 16;
constexpr int kMaxR = ADAPTSEG_BLUR_MAX_RADIUS;
constexpr int kStageW = kTileW + 2 * kMaxR;   // 78: the staged planes' row pitch, whatever R
constexpr int kStageH = kTileH + 2 * kMaxR;   // 30
constexpr int kPixPerBlock = kTileW * kTileH; // 1024 = 256 threads x 4 pixels on the per-pixel path

struct AugArgs {
  int h, w, vec;
  float mean_b, mean_g, mean_r;
  const float *in;
  const int32_t *ctl;      // [n][4]: jitter flag, order code, radius, 0
  const float *jit;        // [n][4]: db, fc, fs, fh
  const float *weights;    // [n][8]: the half kernel
  float *out;
};

struct Jitter {
  float db, fc, fs, fh;
  int order;
};

__device__ __forceinline__ float clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }
__device__ __forceinline__ float max2(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float min2(float a, float b) { return a < b ? a : b; }

__device__ __forceinline__ void rgb_to_hsv(float r, float g, float b, float &h, float &s, float &v) {
  const float mx = max2(max2(r, g), b);
  const float mn = min2(min2(r, g), b);
  const float d = mx - mn;
  s = mx > 0.f ? d / (mx > 0.f ? mx : 1.f) : 0.f;
  const float dd = d == 0.f ? 1.f : d;
  float h6 = d == 0.f ? 0.f : (mx == r ? (g - b) / dd : (mx == g ? 2.f + (b - r) / dd : 4.f + (r - g) / dd));
  h6 = h6 < 0.f ? h6 + 6.f : h6;
  h = h6 / 6.f;
  v = mx;
}

__device__ __forceinline__ void hsv_to_rgb(float h, float s, float v, float &r, float &g, float &b) {
  const float h6 = h * 6.f;
  float i = floorf(h6);
  const float f = h6 - i;
  i = i >= 6.f ? 0.f : i;   // h == 1 (f == 0): the colour of h == 0
  const float p = v * (1.f - s);
  const float q = v * (1.f - s * f);
  const float t = v * (1.f - s * (1.f - f));
  r = i == 0.f ? v : (i == 1.f ? q : (i == 2.f ? p : (i == 3.f ? p : (i == 4.f ? t : v))));
  g = i == 0.f ? t : (i == 1.f ? v : (i == 2.f ? v : (i == 3.f ? q : p)));
  b = i == 0.f ? p : (i == 1.f ? p : (i == 2.f ? t : (i == 3.f ? v : (i == 4.f ? v : q))));
}

// One pixel (BGR minus mean) through the four ops in the image's order.  `order` is uniform over
// the block: the switch is a scalar branch, the colour stays in registers.  The loop over the four
// slots is kept rolled (one copy of the switch per call site: the code stays within the
// instruction cache).
__device__ __forceinline__ void jitter_pixel(const AugArgs &a, const Jitter &j, float &x0, float &x1, float &x2) {
  float b = (x0 + a.mean_b) / 255.f, g = (x1 + a.mean_g) / 255.f, r = (x2 + a.mean_r) / 255.f;
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    switch ((j.order >> (2 * k)) & 3) {
      case 0:   // brightness
        r = clamp01(r + j.db);
        g = clamp01(g + j.db);
        b = clamp01(b + j.db);
        break;
      case 1:   // contrast
        r = clamp01(r * j.fc);
        g = clamp01(g * j.fc);
        b = clamp01(b * j.fc);
        break;
      case 2: { // saturation
        float h, s, v;
        rgb_to_hsv(r, g, b, h, s, v);
        hsv_to_rgb(h, clamp01(s * j.fs), v, r, g, b);
        break;
      }
      default: { // hue
        float h, s, v;
        rgb_to_hsv(r, g, b, h, s, v);
        h = h + j.fh;
        h = h - floorf(h);
        hsv_to_rgb(h, s, v, r, g, b);
        break;
      }
    }
  }
  x0 = b * 255.f - a.mean_b;
  x1 = g * 255.f - a.mean_g;
  x2 = r * 255.f - a.mean_r;
}

// index in [-(n - 1), 2 (n - 1)] reflected into [0, n) without repeating the edge (-1 -> 1)
__device__ __forceinline__ int reflect(int i, int n) {
  i = i < 0 ? -i : i;
  return i > n - 1 ? 2 * (n - 1) - i : i;
}

__global__ void __launch_bounds__(kAugThreads) strong_augment_kernel(AugArgs a) {
  __shared__ float stage[3][kStageH][kStageW];   // tile + halo, jittered
  __shared__ float hpass[kStageH][kTileW];       // one channel after the horizontal pass
  const int img = blockIdx.y;
  const int tid = threadIdx.x;
  const int on = a.ctl[img * 4 + 0] != 0;
  Jitter j;
  j.order = a.ctl[img * 4 + 1];
  j.db = a.jit[img * 4 + 0];
  j.fc = a.jit[img * 4 + 1];
  j.fs = a.jit[img * 4 + 2];
  j.fh = a.jit[img * 4 + 3];
  // the host has checked its copy of the controls; a device copy that disagrees still cannot
  // index past the image or the staged planes
  int R = a.ctl[img * 4 + 2];
  const int rcap = (a.h < a.w ? a.h : a.w) - 1;
  R = R < 0 ? 0 : (R > kMaxR ? kMaxR : R);
  R = R > rcap ? rcap : R;

  const int hw = a.h * a.w;
  const float *__restrict__ in = a.in + (int64_t)img * 3 * hw;
  float *__restrict__ out = a.out + (int64_t)img * 3 * hw;

  if (R == 0) {   // ---- per-pixel path ----
    const int per_sweep = gridDim.x * kPixPerBlock;
    for (int base = blockIdx.x * kPixPerBlock; base < hw; base += per_sweep) {
      if (a.vec) {
        const int i = base + tid * 4;
        if (i < hw) {   // hw % 4 == 0: a whole quad
          float4 c0 = *reinterpret_cast<const float4 *>(in + i);
          float4 c1 = *reinterpret_cast<const float4 *>(in + hw + i);
          float4 c2 = *reinterpret_cast<const float4 *>(in + 2 * (int64_t)hw + i);
          if (on) {
            jitter_pixel(a, j, c0.x, c1.x, c2.x);
            jitter_pixel(a, j, c0.y, c1.y, c2.y);
            jitter_pixel(a, j, c0.z, c1.z, c2.z);
            jitter_pixel(a, j, c0.w, c1.w, c2.w);
          }
          *reinterpret_cast<float4 *>(out + i) = c0;
          *reinterpret_cast<float4 *>(out + hw + i) = c1;
          *reinterpret_cast<float4 *>(out + 2 * (int64_t)hw + i) = c2;
        }
      } else {
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
          const int i = base + k * kAugThreads + tid;
          if (i < hw) {
            float c0 = in[i], c1 = in[hw + i], c2 = in[2 * (int64_t)hw + i];
            if (on) jitter_pixel(a, j, c0, c1, c2);
            out[i] = c0;
            out[hw + i] = c1;
            out[2 * (int64_t)hw + i] = c2;
          }
        }
      }
    }
    return;
  }

  // ---- tile path ----
  const int tiles_x = (a.w + kTileW - 1) / kTileW;
  const int tiles_y = (a.h + kTileH - 1) / kTileH;
  const int sh = kTileH + 2 * R, sw = kTileW + 2 * R;
  const float *__restrict__ wk = a.weights + img * 8;
  const float w0 = wk[0];
  for (int tile = blockIdx.x; tile < tiles_x * tiles_y; tile += gridDim.x) {
    const int ty0 = (tile / tiles_x) * kTileH, tx0 = (tile % tiles_x) * kTileW;
    // stage: rows [ty0 - R, ty0 + 16 + R), columns [tx0 - R, tx0 + 64 + R), reflected at the borders;
    // positions no output of the image needs (past its last row / column + R) hold zeros
    for (int e = tid; e < sh * kStageW; e += kAugThreads) {
      const int sy = e / kStageW, sx = e - sy * kStageW;
      if (sx >= sw) continue;
      const int ry = ty0 - R + sy, rx = tx0 - R + sx;
      float c0 = 0.f, c1 = 0.f, c2 = 0.f;
      if (ry <= a.h - 1 + R && rx <= a.w - 1 + R) {
        const int p = reflect(ry, a.h) * a.w + reflect(rx, a.w);
        c0 = in[p];
        c1 = in[hw + p];
        c2 = in[2 * (int64_t)hw + p];
        if (on) jitter_pixel(a, j, c0, c1, c2);
      }
      stage[0][sy][sx] = c0;
      stage[1][sy][sx] = c1;
      stage[2][sy][sx] = c2;
    }
    __syncthreads();
    for (int ch = 0; ch < 3; ++ch) {
      // horizontal: every staged row, the tile's 64 columns
      for (int e = tid; e < sh * kTileW; e += kAugThreads) {
        const int sy = e / kTileW, c = e % kTileW;
        const float *row = &stage[ch][sy][c + R];
        float acc = w0 * row[0];
        for (int d = 1; d <= R; ++d) acc = acc + wk[d] * (row[-d] + row[d]);
        hpass[sy][c] = acc;
      }
      __syncthreads();
      // vertical: four rows per thread, a wave on 64 consecutive columns
      const int c = tid % kTileW;
#pragma unroll
      for (int k = 0; k < kTileH / 4; ++k) {
        const int r = tid / kTileW + 4 * k;
        float acc = w0 * hpass[r + R][c];
        for (int d = 1; d <= R; ++d) acc = acc + wk[d] * (hpass[r + R - d][c] + hpass[r + R + d][c]);
        const int y = ty0 + r, x = tx0 + c;
        if (y < a.h && x < a.w) out[(int64_t)ch * hw + y * a.w + x] = acc;
      }
      __syncthreads();   // hpass (and, after the last channel, stage) is rewritten next
    }
  }
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

}  // namespace adaptseg

using namespace adaptseg;

extern "C" {

int adaptseg_strong_augment(int n, int h, int w, const float *images_in, const float *mean, const int32_t *ctl_host,
                            const int32_t *ctl, const float *jitter, const float *weights, float *images_out,
                            adaptseg_stream_t stream) {
  const char *name = "strong_augment";
  AS_CHECK_ARG(n >= 1 && h >= 1 && w >= 1, "%s: bad shape n %d, h %d, w %d", name, n, h, w);
  AS_CHECK_ARG((int64_t)h * w < (1 << 24), "%s: %d x %d pixels per image (expected h * w < 2^24)", name, h, w);
  AS_CHECK_ARG(n <= 65535, "%s: bad n %d (at most 65535 images per call)", name, n);
  AS_CHECK_ARG(images_in && mean && ctl_host && ctl && jitter && weights && images_out,
               "%s: bad args (null pointer)", name);
  AS_CHECK_ARG(images_in != images_out, "%s: images_out is images_in (the blur reads its neighbours: not in place)",
               name);
  const int rcap = (h < w ? h : w) - 1;
  for (int i = 0; i < n; ++i) {
    const int32_t *c = ctl_host + 4 * i;
    AS_CHECK_ARG(c[2] >= 0 && c[2] <= ADAPTSEG_BLUR_MAX_RADIUS, "%s: image %d: bad radius %d (0..%d)", name, i, c[2],
                 ADAPTSEG_BLUR_MAX_RADIUS);
    AS_CHECK_ARG(c[2] <= rcap, "%s: image %d: radius %d on a %d x %d image (the reflection needs R <= min(h, w) - 1)",
                 name, i, c[2], h, w);
    int seen = 0;
    for (int k = 0; k < 4; ++k) seen |= 1 << ((c[1] >> (2 * k)) & 3);
    AS_CHECK_ARG(c[1] >= 0 && c[1] < 256 && seen == 15,
                 "%s: image %d: order code %d is not a permutation of the four ops (2 bits each)", name, i, c[1]);
  }
  AugArgs a;
  a.h = h;
  a.w = w;
  a.vec = ((int64_t)h * w) % 4 == 0 && aligned16(images_in) && aligned16(images_out);
  a.mean_b = mean[0];
  a.mean_g = mean[1];
  a.mean_r = mean[2];
  a.in = images_in;
  a.ctl = ctl;
  a.jit = jitter;
  a.weights = weights;
  a.out = images_out;
  // a tile is 1024 pixels, the per-pixel path's share of a block: one grid serves both paths
  const int64_t tiles = ceil_div(w, kTileW) * ceil_div(h, kTileH);
  strong_augment_kernel<<<dim3((unsigned)tiles, (unsigned)n), kAugThreads, 0, as_stream(stream)>>>(a);
  AS_CHECK_LAUNCH(name);
  return ADAPTSEG_OK;
}

}  // extern "C"
