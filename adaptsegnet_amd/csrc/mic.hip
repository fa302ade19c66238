// Masked Image Consistency (MIC) on the mean teacher's labels: the masking of a target batch.
//   conf_count   per image: the number of target pixels whose confidence reaches tau (classmix_stats's nconf)
//   patch_mask   per image: square patches blanked by the caller's keys (one uint32 per patch, compared with an
//                integer threshold), the teacher's class map as int64 labels, and the confidence weight q with
//                the ignored top / bottom rows zeroed
// HBM-bound passes: 16-byte accesses where the row length and the alignment allow, integer atomics only, the
// keys read through the caches (a grid of any size: nothing is staged in LDS).
#include "common.hpp"

namespace adaptseg {

namespace {

constexpr int kMicThreads = 256;
constexpr int kMicVec = 4;   // pixels per thread and sweep on the vector path

// Blocks per image: one per sweep of 256 threads x 4 pixels, the batch capped at `max_blocks` (a few blocks per
// CU; the grid-stride loop takes the rest).  The count's cap is the smaller one: every block ends with one
// atomic on its image's counter, and those are served one after the other.
inline int mic_grid(int hw, int n, int max_blocks) {
  const int64_t want = ceil_div(hw, kMicThreads * kMicVec);
  const int64_t cap = max_blocks / n > 0 ? max_blocks / n : 1;
  return (int)(want < 1 ? 1 : (want > cap ? cap : want));
}

// grid (blocks, images).  VEC: hw % 4 == 0 and a 16-byte aligned map, 4 pixels per thread and sweep.
template <bool VEC>
__global__ void __launch_bounds__(kMicThreads) conf_count_kernel(int hw, const float *__restrict__ conf, float tau,
                                                                 unsigned int *nconf) {
  __shared__ unsigned int nc;
  const int img = blockIdx.y;
  conf += (int64_t)img * hw;
  if (threadIdx.x == 0) nc = 0u;
  __syncthreads();
  unsigned int mine = 0u;
  const int step = VEC ? kMicVec : 1;
  const int per_sweep = gridDim.x * blockDim.x * step;
  for (int i = (blockIdx.x * blockDim.x + threadIdx.x) * step; i < hw; i += per_sweep) {
    if (VEC) {
      const float4 p = *reinterpret_cast<const float4 *>(conf + i);
      mine += (p.x >= tau) + (p.y >= tau) + (p.z >= tau) + (p.w >= tau);
    } else {
      mine += conf[i] >= tau;
    }
  }
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
  if ((threadIdx.x & (kWave - 1)) == 0 && mine) atomicAdd(&nc, mine);
  __syncthreads();
  if (threadIdx.x == 0 && nc) atomicAdd(&nconf[img], nc);
}

struct MicShape {
  int hw, gw, gpi;       // pixels per image, patch columns, patches per image
  FastDiv w, patch;      // y = i / w, patch row / column = y / patch, x / patch
  int row_lo, row_hi;    // rows y with row_lo <= y < row_hi carry the weight q, the others 0
  int ncls, ignore_label;
  unsigned long long threshold;   // a pixel is masked iff its patch's key < threshold (0 .. 2^32)
};

__device__ __forceinline__ int64_t mic_label(int pred, int ncls, int ignore_label) {
  return pred < ncls ? pred : ignore_label;
}

// The float whose bits are t where the pixel is kept, +0 where it is masked: a select, no arithmetic, so NaN
// payloads and the sign of a zero pass through
__device__ __forceinline__ float keep(bool masked, float t) { return masked ? 0.0f : t; }

// grid (blocks, images).  VEC: w % 4 == 0 (a group of four pixels stays in one row) and aligned maps.
template <bool VEC>
__global__ void __launch_bounds__(kMicThreads) patch_mask_kernel(MicShape s, const float *__restrict__ img_t,
                                                                 const uint8_t *__restrict__ pred_t,
                                                                 const int *__restrict__ nconf,
                                                                 const uint32_t *__restrict__ keys,
                                                                 float *__restrict__ out_img,
                                                                 int64_t *__restrict__ out_lab,
                                                                 float *__restrict__ out_w) {
  const int img = blockIdx.y;
  const int hw = s.hw;
  const float q = (float)nconf[img] / (float)hw;
  keys += (int64_t)img * s.gpi;
  const int64_t pix0 = (int64_t)img * hw;        // first pixel of the image's maps
  const int64_t chan0 = (int64_t)img * 3 * hw;   // first element of its channel 0
  const int step = VEC ? kMicVec : 1;
  const int per_sweep = gridDim.x * blockDim.x * step;
  for (int i = (blockIdx.x * blockDim.x + threadIdx.x) * step; i < hw; i += per_sweep) {
    const int y = (int)fdiv((uint32_t)i, s.w);
    const int x = i - y * (int)s.w.d;
    const uint32_t *krow = keys + (int64_t)fdiv((uint32_t)y, s.patch) * s.gw;
    const float wq = y >= s.row_lo && y < s.row_hi ? q : 0.0f;
    const int px = (int)fdiv((uint32_t)x, s.patch);
    const uint32_t k0 = krow[px];
    if (VEC) {
      // patch % 4 != 0: the group may straddle a patch column, every pixel then looks up its own key
      bool m[kMicVec];
      m[0] = k0 < s.threshold;
#pragma unroll
      for (int j = 1; j < kMicVec; ++j) {
        const int pj = (int)fdiv((uint32_t)(x + j), s.patch);
        m[j] = (pj == px ? k0 : krow[pj]) < s.threshold;
      }
      const uchar4 p = *reinterpret_cast<const uchar4 *>(pred_t + pix0 + i);
      longlong2 o0, o1;
      o0.x = mic_label(p.x, s.ncls, s.ignore_label);
      o0.y = mic_label(p.y, s.ncls, s.ignore_label);
      o1.x = mic_label(p.z, s.ncls, s.ignore_label);
      o1.y = mic_label(p.w, s.ncls, s.ignore_label);
      *reinterpret_cast<longlong2 *>(out_lab + pix0 + i) = o0;
      *reinterpret_cast<longlong2 *>(out_lab + pix0 + i + 2) = o1;
      *reinterpret_cast<float4 *>(out_w + pix0 + i) = make_float4(wq, wq, wq, wq);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int64_t e = chan0 + (int64_t)ch * hw + i;
        const float4 t = *reinterpret_cast<const float4 *>(img_t + e);
        *reinterpret_cast<float4 *>(out_img + e) =
            make_float4(keep(m[0], t.x), keep(m[1], t.y), keep(m[2], t.z), keep(m[3], t.w));
      }
    } else {
      const bool m = k0 < s.threshold;
      out_lab[pix0 + i] = mic_label(pred_t[pix0 + i], s.ncls, s.ignore_label);
      out_w[pix0 + i] = wq;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int64_t e = chan0 + (int64_t)ch * hw + i;
        out_img[e] = keep(m, img_t[e]);
      }
    }
  }
}

inline bool mic_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The shape checks the two entry points share (before the pointer checks, before any launch)
int mic_shape_ok(const char *name, int n, int h, int w) {
  AS_CHECK_ARG(n >= 1 && h >= 1 && w >= 1, "%s: bad shape n %d, h %d, w %d", name, n, h, w);
  AS_CHECK_ARG((int64_t)h * w < (1 << 24), "%s: %d x %d pixels per image (expected h * w < 2^24)", name, h, w);
  AS_CHECK_ARG(n <= 65535, "%s: bad n %d (at most 65535 images per call)", name, n);
  return ADAPTSEG_OK;
}

}  // namespace

}  // namespace adaptseg

using namespace adaptseg;

extern "C" {

int adaptseg_conf_count(int n, int h, int w, const float *conf_t, float tau, int32_t *nconf,
                        adaptseg_stream_t stream) {
  if (int st = mic_shape_ok("conf_count", n, h, w)) return st;
  AS_CHECK_ARG(conf_t && nconf, "conf_count: bad args (null pointer)");
  const int hw = h * w;
  hipStream_t s = as_stream(stream);
  if (hipMemsetAsync(nconf, 0, (size_t)n * sizeof(int32_t), s) != hipSuccess) {
    set_error("conf_count: clearing the counts failed: %s", hipGetErrorString(hipGetLastError()));
    return ADAPTSEG_ERR_HIP;
  }
  unsigned int *nc = reinterpret_cast<unsigned int *>(nconf);
  const dim3 grid((unsigned)mic_grid(hw, n, ADAPTSEG_MIC_COUNT_MAX_BLOCKS), (unsigned)n);
  if (hw % kMicVec == 0 && mic_aligned16(conf_t))
    conf_count_kernel<true><<<grid, kMicThreads, 0, s>>>(hw, conf_t, tau, nc);
  else
    conf_count_kernel<false><<<grid, kMicThreads, 0, s>>>(hw, conf_t, tau, nc);
  AS_CHECK_LAUNCH("conf_count");
  return ADAPTSEG_OK;
}

int adaptseg_patch_mask(int n, int h, int w, int patch, int64_t threshold, int num_classes, int ignore_label,
                        int ignore_top, int ignore_bottom, const float *images_t, const uint8_t *pred_t,
                        const int32_t *nconf, const uint32_t *keys, float *masked_images, int64_t *labels,
                        float *weights, adaptseg_stream_t stream) {
  if (int st = mic_shape_ok("patch_mask", n, h, w)) return st;
  AS_CHECK_ARG(patch >= 1, "patch_mask: bad patch %d (at least 1)", patch);
  AS_CHECK_ARG(threshold >= 0 && threshold <= (1ll << 32), "patch_mask: bad threshold %lld (0 .. 2^32)",
               (long long)threshold);
  AS_CHECK_ARG(num_classes >= 1 && num_classes <= 256, "patch_mask: bad num_classes %d (1..256)", num_classes);
  AS_CHECK_ARG(ignore_label >= 0 && ignore_label <= 255, "patch_mask: bad ignore_label %d (0..255)", ignore_label);
  AS_CHECK_ARG(ignore_top >= 0 && ignore_bottom >= 0, "patch_mask: bad ignore rows, top %d, bottom %d (at least 0)",
               ignore_top, ignore_bottom);
  AS_CHECK_ARG(images_t && pred_t && nconf && keys && masked_images && labels && weights,
               "patch_mask: bad args (null pointer)");
  MicShape s;
  s.hw = h * w;
  s.gw = (int)ceil_div(w, patch);
  s.gpi = (int)ceil_div(h, patch) * s.gw;
  s.w = make_fastdiv((uint32_t)w);
  s.patch = make_fastdiv((uint32_t)patch);
  s.row_lo = ignore_top < h ? ignore_top : h;
  s.row_hi = ignore_bottom < h ? h - ignore_bottom : 0;
  s.ncls = num_classes;
  s.ignore_label = ignore_label;
  s.threshold = (unsigned long long)threshold;
  const dim3 grid((unsigned)mic_grid(s.hw, n, ADAPTSEG_MIC_MAX_BLOCKS), (unsigned)n);
  const bool vec = w % kMicVec == 0 && mic_aligned16(images_t) && (reinterpret_cast<uintptr_t>(pred_t) & 3u) == 0 &&
                   mic_aligned16(masked_images) && mic_aligned16(labels) && mic_aligned16(weights);
  if (vec)
    patch_mask_kernel<true><<<grid, kMicThreads, 0, as_stream(stream)>>>(s, images_t, pred_t, nconf, keys,
                                                                         masked_images, labels, weights);
  else
    patch_mask_kernel<false><<<grid, kMicThreads, 0, as_stream(stream)>>>(s, images_t, pred_t, nconf, keys,
                                                                          masked_images, labels, weights);
  AS_CHECK_LAUNCH("patch_mask");
  return ADAPTSEG_OK;
}

}  // extern "C"
