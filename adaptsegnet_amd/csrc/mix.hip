// Online self-training (the DACS recipe): the mean teacher's EMA update and ClassMix.
//   ema / ema_multi   dst = fmaf(alpha, dst, (1 - alpha) * src) over an arena / a table of small tensors
//   classmix_stats    per image: source-label counts per class and the number of confident target pixels
//   classmix_apply    per image: the class selection (recomputed by every block from the counts and the
//                     caller's keys, so nothing returns to the host), then the pasted image, labels, weights
// HBM-bound passes: 16-byte accesses where the alignment allows, integer atomics only.
#include "common.hpp"

namespace adaptseg {

namespace {

constexpr int kMixThreads = 256;
constexpr int kMixVec = 4;   // elements (pixels) per thread and sweep

// ------------------------------------------------------------------------------------
// EMA
// ------------------------------------------------------------------------------------
// a == 0 stores the source's bits (fmaf(0, d, s) would turn a -0 source into +0 and a non-finite
// d into NaN); a == 1 never gets here.  The product b * s is rounded on its own, then one fmaf.
__device__ __forceinline__ float ema1(float a, float b, float d, float s) {
  return a == 0.f ? s : fmaf(a, d, b * s);
}

template <bool VEC>
__global__ void __launch_bounds__(kMixThreads) ema_kernel(int64_t n, float a, float b, const float *__restrict__ src,
                                                          float *__restrict__ dst) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  if (VEC) {
    const int64_t n4 = n / kMixVec;
    const float4 *s4 = reinterpret_cast<const float4 *>(src);
    float4 *d4 = reinterpret_cast<float4 *>(dst);
    for (int64_t i = tid; i < n4; i += nthreads) {
      const float4 s = s4[i];
      float4 d = d4[i];
      d.x = ema1(a, b, d.x, s.x);
      d.y = ema1(a, b, d.y, s.y);
      d.z = ema1(a, b, d.z, s.z);
      d.w = ema1(a, b, d.w, s.w);
      d4[i] = d;
    }
    for (int64_t i = n4 * kMixVec + tid; i < n; i += nthreads) dst[i] = ema1(a, b, dst[i], src[i]);   // the tail
  } else {
    for (int64_t i = tid; i < n; i += nthreads) dst[i] = ema1(a, b, dst[i], src[i]);
  }
}

// Up to ADAPTSEG_EMA_CHUNK tensors per launch, their pointers and lengths kernel arguments
// (data.hip's AugChunk): grid (blocks, tensors of the chunk), indexed by the uniform blockIdx.y.
struct EmaChunk {
  const float *src[ADAPTSEG_EMA_CHUNK];
  float *dst[ADAPTSEG_EMA_CHUNK];
  int n[ADAPTSEG_EMA_CHUNK];
};

__global__ void __launch_bounds__(kMixThreads) ema_multi_kernel(EmaChunk c, float a, float b) {
  const int t = blockIdx.y;
  const int n = c.n[t];
  const float *__restrict__ src = c.src[t];
  float *__restrict__ dst = c.dst[t];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    dst[i] = ema1(a, b, dst[i], src[i]);
}

// ------------------------------------------------------------------------------------
// ClassMix
// ------------------------------------------------------------------------------------
inline int mix_grid(int hw) {
  const int64_t b = ceil_div(hw, kMixThreads * kMixVec);
  return (int)(b < 1 ? 1 : (b > ADAPTSEG_CLASSMIX_MAX_BLOCKS ? ADAPTSEG_CLASSMIX_MAX_BLOCKS : b));
}

// bins[key] += 1 for every lane with key >= 0, called by all 64 lanes of a wave together: label
// maps put most of a wave on one class, and equal addresses of one atomic wave-instruction are
// served one after the other, so twice the first pending lane's key is broadcast, the lanes that
// share it are counted with a ballot and that lane adds the count alone (pseudo.hip's wave_count).
__device__ __forceinline__ void wave_count(unsigned int *bins, int key) {
  const int lane = threadIdx.x & (kWave - 1);
  bool todo = key >= 0;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const unsigned long long pending = __ballot(todo);
    if (pending == 0ull) return;
    const int leader = __ffsll((long long)pending) - 1;
    const int k0 = __shfl(key, leader);
    const bool same = todo && key == k0;
    const unsigned long long group = __ballot(same);
    if (lane == leader) atomicAdd(&bins[k0], (unsigned int)__popcll(group));
    todo = todo && !same;
  }
  if (todo) atomicAdd(&bins[key], 1u);
}

__device__ __forceinline__ int label_key(int64_t lab, int ncls) { return lab >= 0 && lab < ncls ? (int)lab : -1; }

// grid (blocks, images).  Every thread of a block runs the same number of sweeps (wave_count is a
// wave-wide call).  VEC: hw % 4 == 0 and 16-byte aligned maps, 4 pixels per thread and sweep.
template <bool VEC>
__global__ void __launch_bounds__(kMixThreads) classmix_stats_kernel(int hw, int ncls,
                                                                     const int64_t *__restrict__ labels,
                                                                     const float *__restrict__ conf, float tau,
                                                                     unsigned int *count, unsigned int *nconf) {
  __shared__ unsigned int cnt[256];
  __shared__ unsigned int nc;
  const int img = blockIdx.y;
  labels += (int64_t)img * hw;
  conf += (int64_t)img * hw;
  for (int j = threadIdx.x; j < 256; j += blockDim.x) cnt[j] = 0u;
  if (threadIdx.x == 0) nc = 0u;
  __syncthreads();
  unsigned int mine = 0u;
  const int step = VEC ? kMixVec : 1;
  const int per_sweep = gridDim.x * blockDim.x * step;
  for (int base = blockIdx.x * blockDim.x * step; base < hw; base += per_sweep) {
    const int i = base + threadIdx.x * step;
    if (VEC) {
      int key[kMixVec] = {-1, -1, -1, -1};
      if (i < hw) {
        const longlong2 l0 = *reinterpret_cast<const longlong2 *>(labels + i);
        const longlong2 l1 = *reinterpret_cast<const longlong2 *>(labels + i + 2);
        const float4 p = *reinterpret_cast<const float4 *>(conf + i);
        key[0] = label_key(l0.x, ncls);
        key[1] = label_key(l0.y, ncls);
        key[2] = label_key(l1.x, ncls);
        key[3] = label_key(l1.y, ncls);
        mine += (p.x >= tau) + (p.y >= tau) + (p.z >= tau) + (p.w >= tau);
      }
#pragma unroll
      for (int j = 0; j < kMixVec; ++j) wave_count(cnt, key[j]);
    } else {
      int key = -1;
      if (i < hw) {
        key = label_key(labels[i], ncls);
        mine += conf[i] >= tau;
      }
      wave_count(cnt, key);
    }
  }
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
  if ((threadIdx.x & (kWave - 1)) == 0 && mine) atomicAdd(&nc, mine);
  __syncthreads();
  for (int j = threadIdx.x; j < ncls; j += blockDim.x)
    if (cnt[j]) atomicAdd(&count[(int64_t)img * ncls + j], cnt[j]);
  if (threadIdx.x == 0 && nc) atomicAdd(&nconf[img], nc);
}

__device__ __forceinline__ float pick(bool m, float s, float t) { return m ? s : t; }

// One pixel's outputs from its source label, the selection and the target prediction
__device__ __forceinline__ bool mix_pixel(int64_t lab, int pred, const unsigned char *sel, int ncls, int ignore_label,
                                          float q, int64_t &out_label, float &out_weight) {
  const bool m = lab >= 0 && lab < ncls && sel[lab];
  out_label = m ? lab : (pred < ncls ? pred : ignore_label);
  out_weight = m ? 1.0f : q;
  return m;
}

template <bool VEC>
__global__ void __launch_bounds__(kMixThreads) classmix_apply_kernel(
    int hw, int ncls, const float *__restrict__ img_s, const int64_t *__restrict__ lab_s,
    const float *__restrict__ img_t, const uint8_t *__restrict__ pred_t, const int *__restrict__ count,
    const int *__restrict__ nconf, const uint32_t *__restrict__ keys, int ignore_label, float *__restrict__ out_img,
    int64_t *__restrict__ out_lab, float *__restrict__ out_w, uint8_t *__restrict__ mask) {
  __shared__ uint32_t skey[256];
  __shared__ unsigned char spres[256];
  __shared__ unsigned char sel[256];
  const int img = blockIdx.y;
  // the selection: class c (thread c) is selected when it is present and fewer than ceil(k / 2)
  // present classes have a smaller (key, index) pair
  for (int c = threadIdx.x; c < 256; c += blockDim.x) {
    const bool in = c < ncls;
    skey[c] = in ? keys[(int64_t)img * ncls + c] : 0u;
    spres[c] = in && count[(int64_t)img * ncls + c] > 0;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 256; c += blockDim.x) {
    int k = 0, rank = 0;
    const uint32_t kc = skey[c];
    for (int j = 0; j < ncls; ++j) {
      const bool pj = spres[j];
      k += pj;
      rank += pj && (skey[j] < kc || (skey[j] == kc && j < c));
    }
    sel[c] = spres[c] && rank < (k + 1) / 2;
  }
  __syncthreads();
  if (mask && blockIdx.x == 0)
    for (int c = threadIdx.x; c < ncls; c += blockDim.x) mask[(int64_t)img * ncls + c] = sel[c];
  const float q = (float)nconf[img] / (float)hw;

  const int64_t pix0 = (int64_t)img * hw;        // first pixel of the image's maps
  const int64_t chan0 = (int64_t)img * 3 * hw;   // first element of its channel 0
  const int step = VEC ? kMixVec : 1;
  const int per_sweep = gridDim.x * blockDim.x * step;
  for (int i = (blockIdx.x * blockDim.x + threadIdx.x) * step; i < hw; i += per_sweep) {
    if (VEC) {
      const longlong2 l0 = *reinterpret_cast<const longlong2 *>(lab_s + pix0 + i);
      const longlong2 l1 = *reinterpret_cast<const longlong2 *>(lab_s + pix0 + i + 2);
      const uchar4 p = *reinterpret_cast<const uchar4 *>(pred_t + pix0 + i);
      longlong2 o0, o1;
      float4 w;
      int64_t ol;
      const bool m0 = mix_pixel(l0.x, p.x, sel, ncls, ignore_label, q, ol, w.x);
      o0.x = ol;
      const bool m1 = mix_pixel(l0.y, p.y, sel, ncls, ignore_label, q, ol, w.y);
      o0.y = ol;
      const bool m2 = mix_pixel(l1.x, p.z, sel, ncls, ignore_label, q, ol, w.z);
      o1.x = ol;
      const bool m3 = mix_pixel(l1.y, p.w, sel, ncls, ignore_label, q, ol, w.w);
      o1.y = ol;
      *reinterpret_cast<longlong2 *>(out_lab + pix0 + i) = o0;
      *reinterpret_cast<longlong2 *>(out_lab + pix0 + i + 2) = o1;
      *reinterpret_cast<float4 *>(out_w + pix0 + i) = w;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int64_t e = chan0 + (int64_t)ch * hw + i;
        const float4 s = *reinterpret_cast<const float4 *>(img_s + e);
        const float4 t = *reinterpret_cast<const float4 *>(img_t + e);
        *reinterpret_cast<float4 *>(out_img + e) =
            make_float4(pick(m0, s.x, t.x), pick(m1, s.y, t.y), pick(m2, s.z, t.z), pick(m3, s.w, t.w));
      }
    } else {
      int64_t ol;
      float w;
      const bool m = mix_pixel(lab_s[pix0 + i], pred_t[pix0 + i], sel, ncls, ignore_label, q, ol, w);
      out_lab[pix0 + i] = ol;
      out_w[pix0 + i] = w;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int64_t e = chan0 + (int64_t)ch * hw + i;
        out_img[e] = pick(m, img_s[e], img_t[e]);
      }
    }
  }
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The shape checks the two ClassMix entry points share (before the pointer checks, before any launch)
int classmix_shape_ok(const char *name, int n, int h, int w, int ncls) {
  AS_CHECK_ARG(ncls >= 1 && ncls <= 256, "%s: bad ncls %d (1..256)", name, ncls);
  AS_CHECK_ARG(n >= 1 && h >= 1 && w >= 1, "%s: bad shape n %d, h %d, w %d", name, n, h, w);
  AS_CHECK_ARG((int64_t)h * w < (1 << 24), "%s: %d x %d pixels per image (expected h * w < 2^24)", name, h, w);
  AS_CHECK_ARG(n <= 65535, "%s: bad n %d (at most 65535 images per call)", name, n);
  return ADAPTSEG_OK;
}

int ema_args_ok(const char *name, float alpha) {
  AS_CHECK_ARG(alpha >= 0.f && alpha <= 1.f, "%s: bad alpha %g (0 <= alpha <= 1)", name, (double)alpha);
  return ADAPTSEG_OK;
}

}  // namespace

}  // namespace adaptseg

using namespace adaptseg;

extern "C" {

int adaptseg_ema(int64_t n, float alpha, const float *src, float *dst, adaptseg_stream_t stream) {
  AS_CHECK_ARG(n >= 0, "ema: bad n %lld", (long long)n);
  if (int st = ema_args_ok("ema", alpha)) return st;
  AS_CHECK_ARG(n == 0 || (src && dst), "ema: bad args (null pointer)");
  if (n == 0 || alpha == 1.f) return ADAPTSEG_OK;
  const float beta = 1.f - alpha;
  const bool vec = aligned16(src) && aligned16(dst);
  const int64_t b = ceil_div(vec ? ceil_div(n, kMixVec) : n, kMixThreads);
  const int grid = (int)(b > ADAPTSEG_EMA_MAX_BLOCKS ? ADAPTSEG_EMA_MAX_BLOCKS : b);
  if (vec) ema_kernel<true><<<grid, kMixThreads, 0, as_stream(stream)>>>(n, alpha, beta, src, dst);
  else ema_kernel<false><<<grid, kMixThreads, 0, as_stream(stream)>>>(n, alpha, beta, src, dst);
  AS_CHECK_LAUNCH("ema");
  return ADAPTSEG_OK;
}

int adaptseg_ema_multi(int count, const float *const *src, float *const *dst, const int64_t *n, float alpha,
                       adaptseg_stream_t stream) {
  AS_CHECK_ARG(count >= 0, "ema_multi: bad count %d", count);
  if (int st = ema_args_ok("ema_multi", alpha)) return st;
  AS_CHECK_ARG(count == 0 || (src && dst && n), "ema_multi: bad args (null table)");
  for (int i = 0; i < count; ++i) {
    AS_CHECK_ARG(n[i] >= 0 && n[i] < (1ll << 31), "ema_multi: tensor %d has %lld elements (0 .. 2^31 - 1)", i,
                 (long long)n[i]);
    AS_CHECK_ARG(n[i] == 0 || (src[i] && dst[i]), "ema_multi: tensor %d: null pointer", i);
  }
  if (count == 0 || alpha == 1.f) return ADAPTSEG_OK;
  const float beta = 1.f - alpha;
  for (int first = 0; first < count; first += ADAPTSEG_EMA_CHUNK) {
    const int m = count - first < ADAPTSEG_EMA_CHUNK ? count - first : ADAPTSEG_EMA_CHUNK;
    EmaChunk c = {};
    int64_t longest = 0;
    for (int i = 0; i < m; ++i) {
      c.src[i] = src[first + i];
      c.dst[i] = dst[first + i];
      c.n[i] = (int)n[first + i];
      if (n[first + i] > longest) longest = n[first + i];
    }
    if (longest == 0) continue;
    const int64_t b = ceil_div(longest, kMixThreads);
    ema_multi_kernel<<<dim3((unsigned)(b > 64 ? 64 : b), (unsigned)m), kMixThreads, 0, as_stream(stream)>>>(c, alpha,
                                                                                                            beta);
    AS_CHECK_LAUNCH("ema_multi");
  }
  return ADAPTSEG_OK;
}

int adaptseg_classmix_stats(int n, int h, int w, int ncls, const int64_t *labels_s, const float *conf_t, float tau,
                            int32_t *count, int32_t *nconf, adaptseg_stream_t stream) {
  if (int st = classmix_shape_ok("classmix_stats", n, h, w, ncls)) return st;
  AS_CHECK_ARG(labels_s && conf_t && count && nconf, "classmix_stats: bad args (null pointer)");
  const int hw = h * w;
  hipStream_t s = as_stream(stream);
  if (hipMemsetAsync(count, 0, (size_t)n * ncls * sizeof(int32_t), s) != hipSuccess ||
      hipMemsetAsync(nconf, 0, (size_t)n * sizeof(int32_t), s) != hipSuccess) {
    set_error("classmix_stats: clearing the counts failed: %s", hipGetErrorString(hipGetLastError()));
    return ADAPTSEG_ERR_HIP;
  }
  unsigned int *cnt = reinterpret_cast<unsigned int *>(count), *nc = reinterpret_cast<unsigned int *>(nconf);
  const dim3 grid((unsigned)mix_grid(hw), (unsigned)n);
  if (hw % kMixVec == 0 && aligned16(labels_s) && aligned16(conf_t))
    classmix_stats_kernel<true><<<grid, kMixThreads, 0, s>>>(hw, ncls, labels_s, conf_t, tau, cnt, nc);
  else
    classmix_stats_kernel<false><<<grid, kMixThreads, 0, s>>>(hw, ncls, labels_s, conf_t, tau, cnt, nc);
  AS_CHECK_LAUNCH("classmix_stats");
  return ADAPTSEG_OK;
}

int adaptseg_classmix_apply(int n, int h, int w, int ncls, const float *images_s, const int64_t *labels_s,
                            const float *images_t, const uint8_t *pred_t, const int32_t *count, const int32_t *nconf,
                            const uint32_t *keys, int ignore_label, float *mixed_images, int64_t *mixed_labels,
                            float *mixed_weights, uint8_t *mask, adaptseg_stream_t stream) {
  if (int st = classmix_shape_ok("classmix_apply", n, h, w, ncls)) return st;
  AS_CHECK_ARG(ignore_label >= 0 && ignore_label <= 255, "classmix_apply: bad ignore_label %d (0..255)", ignore_label);
  AS_CHECK_ARG(images_s && labels_s && images_t && pred_t && count && nconf && keys && mixed_images && mixed_labels &&
                   mixed_weights,
               "classmix_apply: bad args (null pointer)");
  const int hw = h * w;
  const dim3 grid((unsigned)mix_grid(hw), (unsigned)n);
  const bool vec = hw % kMixVec == 0 && aligned16(images_s) && aligned16(labels_s) && aligned16(images_t) &&
                   (reinterpret_cast<uintptr_t>(pred_t) & 3u) == 0 && aligned16(mixed_images) &&
                   aligned16(mixed_labels) && aligned16(mixed_weights);
  if (vec)
    classmix_apply_kernel<true><<<grid, kMixThreads, 0, as_stream(stream)>>>(
        hw, ncls, images_s, labels_s, images_t, pred_t, count, nconf, keys, ignore_label, mixed_images, mixed_labels,
        mixed_weights, mask);
  else
    classmix_apply_kernel<false><<<grid, kMixThreads, 0, as_stream(stream)>>>(
        hw, ncls, images_s, labels_s, images_t, pred_t, count, nconf, keys, ignore_label, mixed_images, mixed_labels,
        mixed_weights, mask);
  AS_CHECK_LAUNCH("classmix_apply");
  return ADAPTSEG_OK;
}

}  // extern "C"
