// FDA (Fourier Domain Adaptation, Yang & Soatto, CVPR 2020) spectral transfer: the low-frequency
// amplitude spectrum of every source image is replaced by its target image's, the phase stays.
// Only the (2b+1)^2 coefficients with |u|, |v| <= b change, and for real images the result is the
// source plus a real low-frequency correction:
//   out = src + (1/HW) sum_{|u|,|v|<=b} D(u,v) e^{+2 pi i (uy/H + vx/W)},  D = (|T| - |S|) S/|S|
// so no full FFT runs: a separable partial DFT of both images, then a separable synthesis.
//   fda_rows   R(y,v) = sum_x img(y,x) e^{-2 pi i vx/W}, v = 0..b (v < 0 by conjugation), both images.
//              A block: a tile of rows of one image-channel; a thread: one (row, v); the row chunk
//              (source and target interleaved) and the W twiddles sit in LDS.  fp32 sums over
//              chunks of 256 columns in column order, the chunk sums added in fp64 in chunk order.
//   fda_cols   F(u,v) = sum_y R(y,v) e^{-2 pi i uy/H}, u = -b..b, in fp64: a block per (u, image-
//              channel), wave s sums the rows y = s mod 4 in row order, wave 0 adds the four
//              slices in slice order, adds mean H W to the DC terms, and forms
//              D(u,v) w_v / (H W) (w_0 = 1, w_v = 2: the v < 0 half folded in).
//   fda_g      G(y,v) = sum_u D(u,v) e^{+2 pi i uy/H} in fp64, u ascending.
//   fda_apply  out = src + sum_v Re(G(y,v) e^{+2 pi i vx/W}), fp32, v DEscending (the small
//              high-frequency terms first, the DC shift last).  A thread: one column of 8 rows, so
//              a twiddle read serves 8 pixels; G(y,v) is uniform over the block.
// The twiddles come from the caller's tables (cos, sin)(2 pi k / n), indexed by the integer
// (v x) mod W kept incrementally: no sincos on the device.  Every sum has a fixed order and reads
// only its own image-channel: the result does not depend on N or on the image's place in the batch.
#include "common.hpp"

namespace adaptseg {

namespace {

constexpr int kFdaThreads = 256;
constexpr int kChunk = 256;              // columns per staged chunk of fda_rows
constexpr int kPitch = kChunk + 1;       // float2 words per staged row: rows on different banks
constexpr int kMaxRowTile = 15;          // rows per block of fda_rows (with kMaxW: under 64 KiB of LDS)
constexpr int kMaxW = 4096;              // the W twiddles are held in LDS (32 KiB at most)
constexpr int kApplyRows = 8;            // rows per thread of fda_apply
constexpr int kApplyGroups = 4;          // row groups per block of fda_apply (one table load serves 32 rows)

struct FdaArgs {
  int c, h, w, b, b1;     // b1 = b + 1 frequencies v = 0..b
  int vec;                // 16-byte loads of src / trg rows (w % 4 == 0, both 16-byte aligned)
  int rt, vpb;            // fda_rows: rows per block, frequencies per pass (rt * vpb <= 256)
  const float *src, *trg, *mean;
  const float2 *tw_w, *tw_h;
  float2 *rs, *rt_;       // R of the source / target  [nc][h][b1]
  float2 *g;              // G                          [nc][h][b1]
  float2 *d;              // D w_v / (H W)              [nc][2b+1][b1]
  float *out;
};

__global__ void __launch_bounds__(kFdaThreads) fda_rows_kernel(FdaArgs a) {
  extern __shared__ float2 fda_sm[];
  float2 *tw = fda_sm;            // [w]
  float2 *stage = fda_sm + a.w;   // [rt][kPitch]: (src, trg)
  const int tid = threadIdx.x;
  const int ic = blockIdx.y;
  const int y0 = blockIdx.x * a.rt;
  for (int i = tid; i < a.w; i += kFdaThreads) tw[i] = a.tw_w[i];
  const float *__restrict__ src = a.src + (int64_t)ic * a.h * a.w;
  const float *__restrict__ trg = a.trg + (int64_t)ic * a.h * a.w;
  const int r = tid / a.vpb, vl = tid - r * a.vpb;
  const int y = y0 + r;
  for (int v0 = 0; v0 < a.b1; v0 += a.vpb) {
    const int v = v0 + vl;
    const bool active = r < a.rt && y < a.h && v < a.b1;
    double sre = 0., sim = 0., tre = 0., tim = 0.;
    int idx = 0;   // (v x) mod w
    for (int x0 = 0; x0 < a.w; x0 += kChunk) {
      const int nx = min(kChunk, a.w - x0);
      __syncthreads();   // the last chunk has been read (first pass: the table is written)
      if (a.vec) {
        for (int e = tid; e < a.rt * (kChunk / 4); e += kFdaThreads) {
          const int rr = e / (kChunk / 4), xx = (e % (kChunk / 4)) * 4;
          if (xx < nx && y0 + rr < a.h) {   // w % 4 == 0: a whole quad
            const int64_t p = (int64_t)(y0 + rr) * a.w + x0 + xx;
            const float4 s = *reinterpret_cast<const float4 *>(src + p);
            const float4 t = *reinterpret_cast<const float4 *>(trg + p);
            float2 *o = stage + rr * kPitch + xx;
            o[0] = make_float2(s.x, t.x);
            o[1] = make_float2(s.y, t.y);
            o[2] = make_float2(s.z, t.z);
            o[3] = make_float2(s.w, t.w);
          }
        }
      } else {
        for (int e = tid; e < a.rt * kChunk; e += kFdaThreads) {
          const int rr = e / kChunk, xx = e % kChunk;
          if (xx < nx && y0 + rr < a.h) {
            const int64_t p = (int64_t)(y0 + rr) * a.w + x0 + xx;
            stage[rr * kPitch + xx] = make_float2(src[p], trg[p]);
          }
        }
      }
      __syncthreads();
      if (active) {
        const float2 *row = stage + r * kPitch;
        float ar = 0.f, ai = 0.f, br = 0.f, bi = 0.f;
        for (int x = 0; x < nx; ++x) {
          const float2 t = tw[idx], p = row[x];
          ar = fmaf(p.x, t.x, ar);
          ai = fmaf(p.x, t.y, ai);
          br = fmaf(p.y, t.x, br);
          bi = fmaf(p.y, t.y, bi);
          idx += v;
          idx = idx >= a.w ? idx - a.w : idx;
        }
        sre += (double)ar;   // e^{-i th} = cos th - i sin th
        sim -= (double)ai;
        tre += (double)br;
        tim -= (double)bi;
      }
    }
    if (active) {
      const int64_t o = ((int64_t)ic * a.h + y) * a.b1 + v;
      a.rs[o] = make_float2((float)sre, (float)sim);
      a.rt_[o] = make_float2((float)tre, (float)tim);
    }
  }
}

__global__ void __launch_bounds__(kFdaThreads) fda_cols_kernel(FdaArgs a) {
  __shared__ double red[4][4][kWave];   // [slice][S re, S im, T re, T im][lane]
  const int tid = threadIdx.x, lane = tid & 63, slice = tid >> 6;
  const int ui = blockIdx.x, u = ui - a.b, au = u < 0 ? -u : u;
  const int ic = blockIdx.y;
  const double sgn = u < 0 ? -1. : 1.;   // e^{-2 pi i u y / H} = cos(|u| th) - i sgn(u) sin(|u| th)
  const int step = (4 * au) % a.h;
  const float2 *__restrict__ rs = a.rs + (int64_t)ic * a.h * a.b1;
  const float2 *__restrict__ rt = a.rt_ + (int64_t)ic * a.h * a.b1;
  for (int v0 = 0; v0 < a.b1; v0 += kWave) {
    const int v = v0 + lane;
    double sr = 0., si = 0., tr = 0., ti = 0.;
    if (v < a.b1) {
      int idx = (au * slice) % a.h;   // (|u| y) mod h
      for (int y = slice; y < a.h; y += 4) {
        const float2 t = a.tw_h[idx];
        const double c = (double)t.x, s = sgn * (double)t.y;
        const float2 ps = rs[(int64_t)y * a.b1 + v], pt = rt[(int64_t)y * a.b1 + v];
        // (pr + i pi) (c - i s)
        sr = fma((double)ps.x, c, fma((double)ps.y, s, sr));
        si = fma((double)ps.y, c, fma(-(double)ps.x, s, si));
        tr = fma((double)pt.x, c, fma((double)pt.y, s, tr));
        ti = fma((double)pt.y, c, fma(-(double)pt.x, s, ti));
        idx += step;
        idx = idx >= a.h ? idx - a.h : idx;
      }
    }
    red[slice][0][lane] = sr;
    red[slice][1][lane] = si;
    red[slice][2][lane] = tr;
    red[slice][3][lane] = ti;
    __syncthreads();
    if (slice == 0 && v < a.b1) {
      double f[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) f[k] = ((red[0][k][lane] + red[1][k][lane]) + red[2][k][lane]) + red[3][k][lane];
      if (u == 0 && v == 0 && a.mean) {   // the spectrum of x + mean: only the DC terms see the mean
        const double m = (double)a.mean[ic % a.c] * (double)a.h * (double)a.w;
        f[0] += m;
        f[2] += m;
      }
      const double as = sqrt(f[0] * f[0] + f[1] * f[1]), at = sqrt(f[2] * f[2] + f[3] * f[3]);
      const double pr = as > 0. ? f[0] / as : 1., pi = as > 0. ? f[1] / as : 0.;   // np.angle(0) = 0
      const double k = (at - as) * (v == 0 ? 1. : 2.) / ((double)a.h * (double)a.w);
      a.d[((int64_t)ic * (2 * a.b + 1) + ui) * a.b1 + v] = make_float2((float)(k * pr), (float)(k * pi));
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kFdaThreads) fda_g_kernel(FdaArgs a) {
  const int e = blockIdx.x * kFdaThreads + threadIdx.x;
  const int ic = blockIdx.y;
  if (e >= a.h * a.b1) return;
  const int y = e / a.b1, v = e - y * a.b1;
  const float2 *__restrict__ d = a.d + (int64_t)ic * (2 * a.b + 1) * a.b1 + v;
  int idx = (int)(((uint32_t)a.b * (uint32_t)y) % (uint32_t)a.h);   // (|u| y) mod h at u = -b
  double gr = 0., gi = 0.;
  for (int ui = 0; ui <= 2 * a.b; ++ui) {
    const int u = ui - a.b;
    const float2 t = a.tw_h[idx];
    const double c = (double)t.x, s = u < 0 ? -(double)t.y : (double)t.y;   // e^{+2 pi i u y / H}
    const float2 dd = d[(int64_t)ui * a.b1];
    gr = fma((double)dd.x, c, fma(-(double)dd.y, s, gr));
    gi = fma((double)dd.x, s, fma((double)dd.y, c, gi));
    if (u < 0) {
      idx -= y;
      idx = idx < 0 ? idx + a.h : idx;
    } else {
      idx += y;
      idx = idx >= a.h ? idx - a.h : idx;
    }
  }
  a.g[((int64_t)ic * a.h + y) * a.b1 + v] = make_float2((float)gr, (float)gi);
}

__global__ void __launch_bounds__(kFdaThreads) fda_apply_kernel(FdaArgs a) {
  extern __shared__ float2 fda_sm[];   // [w]
  const int tid = threadIdx.x;
  const int ic = blockIdx.z;
  for (int i = tid; i < a.w; i += kFdaThreads) fda_sm[i] = a.tw_w[i];
  __syncthreads();
  const int x = blockIdx.x * kFdaThreads + tid;
  const bool in = x < a.w;
  const int xc = in ? x : 0;
  const int start = (int)(((uint32_t)a.b * (uint32_t)xc) % (uint32_t)a.w);   // (v x) mod w at v = b
  const float *__restrict__ src = a.src + (int64_t)ic * a.h * a.w;
  float *__restrict__ out = a.out + (int64_t)ic * a.h * a.w;
  const float2 *__restrict__ g = a.g + (int64_t)ic * a.h * a.b1;
  for (int grp = 0; grp < kApplyGroups; ++grp) {
    const int y0 = (blockIdx.y * kApplyGroups + grp) * kApplyRows;
    if (y0 >= a.h) break;
    float s[kApplyRows], acc[kApplyRows];
#pragma unroll
    for (int r = 0; r < kApplyRows; ++r) {
      const int yy = min(y0 + r, a.h - 1);
      s[r] = src[(int64_t)yy * a.w + xc];
      acc[r] = 0.f;
    }
    int idx = start;
    for (int v = a.b; v >= 0; --v) {
      const float2 t = fda_sm[idx];
#pragma unroll
      for (int r = 0; r < kApplyRows; ++r) {
        const int yy = min(y0 + r, a.h - 1);
        const float2 gg = g[(int64_t)yy * a.b1 + v];   // uniform over the block
        acc[r] = fmaf(gg.x, t.x, acc[r]);              // Re(G e^{i th}) = Gr cos th - Gi sin th
        acc[r] = fmaf(-gg.y, t.y, acc[r]);
      }
      idx -= xc;
      idx = idx < 0 ? idx + a.w : idx;
    }
#pragma unroll
    for (int r = 0; r < kApplyRows; ++r)
      if (in && y0 + r < a.h) out[(int64_t)(y0 + r) * a.w + x] = s[r] + acc[r];
  }
}

inline bool aligned_to(const void *p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

inline bool overlaps(const void *p, const void *q, size_t bytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + bytes && b < a + bytes;
}

// shape checks shared by the two entry points
int fda_check_shape(const char *name, int n, int c, int h, int w, int b) {
  AS_CHECK_ARG(n >= 1 && c >= 1 && h >= 1 && w >= 1, "%s: bad shape n %d, c %d, h %d, w %d", name, n, c, h, w);
  AS_CHECK_ARG((int64_t)h * w < (1 << 24), "%s: %d x %d pixels per image (expected h * w < 2^24)", name, h, w);
  AS_CHECK_ARG(w <= kMaxW, "%s: bad w %d (at most %d: the row twiddles are held in LDS)", name, w, kMaxW);
  AS_CHECK_ARG((int64_t)n * c <= 65535, "%s: bad n * c %lld (at most 65535 image-channels per call)", name,
               (long long)n * c);
  AS_CHECK_ARG(b >= 0 && 2 * (int64_t)b + 1 <= (h < w ? h : w),
               "%s: bad b %d on a %d x %d image (expected 0 <= 2 b + 1 <= min(h, w))", name, b, h, w);
  return ADAPTSEG_OK;
}

// workspace: R of the source, R of the target, G (each [nc][h][b+1] float2), D ([nc][2b+1][b+1] float2)
size_t fda_ws_bytes(int n, int c, int h, int b) {
  const size_t nc = (size_t)n * c, b1 = (size_t)b + 1;
  return (3 * nc * h * b1 + nc * (2 * (size_t)b + 1) * b1) * sizeof(float2);
}

}  // namespace

}  // namespace adaptseg

using namespace adaptseg;

extern "C" {

int adaptseg_fda_workspace_size(int n, int c, int h, int w, int b, size_t *bytes) {
  const char *name = "fda_workspace_size";
  AS_CHECK_ARG(bytes, "%s: bad args (null pointer)", name);
  const int st = fda_check_shape(name, n, c, h, w, b);
  if (st != ADAPTSEG_OK) return st;
  *bytes = fda_ws_bytes(n, c, h, b);
  return ADAPTSEG_OK;
}

int adaptseg_fda_transfer(int n, int c, int h, int w, int b, const float *src, const float *trg, const float *mean,
                          const float *tw_w, const float *tw_h, float *out, void *ws, size_t ws_bytes,
                          adaptseg_stream_t stream) {
  const char *name = "fda_transfer";
  const int st = fda_check_shape(name, n, c, h, w, b);
  if (st != ADAPTSEG_OK) return st;
  AS_CHECK_ARG(src && trg && tw_w && tw_h && out, "%s: bad args (null pointer)", name);
  AS_CHECK_ARG(aligned_to(tw_w, 8) && aligned_to(tw_h, 8), "%s: bad twiddle tables (expected 8-byte aligned)", name);
  const size_t img_bytes = (size_t)n * c * h * w * sizeof(float);
  AS_CHECK_ARG(!overlaps(out, src, img_bytes) && !overlaps(out, trg, img_bytes),
               "%s: out aliases src or trg (the synthesis reads src after other rows are written: not in place)", name);
  const size_t need = fda_ws_bytes(n, c, h, b);
  if (!ws || ws_bytes < need || !aligned_to(ws, 8)) {
    set_error("%s: workspace missing, misaligned or too small (%zu bytes, expected %zu, 8-byte aligned)", name,
              ws ? ws_bytes : (size_t)0, need);
    return ADAPTSEG_ERR_WORKSPACE;
  }
  const int nc = n * c;
  FdaArgs a;
  a.c = c;
  a.h = h;
  a.w = w;
  a.b = b;
  a.b1 = b + 1;
  a.vec = w % 4 == 0 && aligned_to(src, 16) && aligned_to(trg, 16);
  a.vpb = a.b1 < kFdaThreads ? a.b1 : kFdaThreads;
  a.rt = kFdaThreads / a.vpb < kMaxRowTile ? kFdaThreads / a.vpb : kMaxRowTile;
  a.rt = a.rt < h ? a.rt : h;
  a.src = src;
  a.trg = trg;
  a.mean = mean;
  a.tw_w = reinterpret_cast<const float2 *>(tw_w);
  a.tw_h = reinterpret_cast<const float2 *>(tw_h);
  const size_t plane = (size_t)nc * h * a.b1;
  a.rs = reinterpret_cast<float2 *>(ws);
  a.rt_ = a.rs + plane;
  a.g = a.rt_ + plane;
  a.d = a.g + plane;
  a.out = out;
  hipStream_t s = as_stream(stream);
  const size_t rows_lds = ((size_t)w + (size_t)a.rt * kPitch) * sizeof(float2);
  fda_rows_kernel<<<dim3((unsigned)ceil_div(h, a.rt), (unsigned)nc), kFdaThreads, rows_lds, s>>>(a);
  AS_CHECK_LAUNCH("fda_rows");
  fda_cols_kernel<<<dim3((unsigned)(2 * b + 1), (unsigned)nc), kFdaThreads, 0, s>>>(a);
  AS_CHECK_LAUNCH("fda_cols");
  fda_g_kernel<<<dim3((unsigned)ceil_div((int64_t)h * a.b1, kFdaThreads), (unsigned)nc), kFdaThreads, 0, s>>>(a);
  AS_CHECK_LAUNCH("fda_g");
  fda_apply_kernel<<<dim3((unsigned)ceil_div(w, kFdaThreads), (unsigned)ceil_div(h, kApplyRows * kApplyGroups),
                          (unsigned)nc),
                     kFdaThreads, (size_t)w * sizeof(float2), s>>>(a);
  AS_CHECK_LAUNCH("fda_apply");
  return ADAPTSEG_OK;
}

}  // extern "C"
