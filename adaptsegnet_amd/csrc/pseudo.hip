// Class-balanced pseudo-labels for self-training (the CBST / BDL recipe) on the outputs of
// adaptseg_fuse_argmax: a per-class histogram of the winning class's confidence, per-class
// thresholds that keep a portion of each class, and the label map they select.  Integer atomics
// only: every count is exact and independent of the order the pixels arrive in.
#include "common.hpp"

namespace adaptseg {

namespace {

constexpr int kPseudoThreads = 256;
// Pixels per block of the histogram / label kernels (256 threads x 16 rounds), as confusion_hist.
constexpr int kPseudoPixPerBlock = kPseudoThreads * 16;
// LDS budget of the block-private histogram: 64 KiB, the dynamic LDS a block gets without opting
// in to more, and two blocks of it still share a CU's 160 KiB.  19 classes x 512 bins are 38 KiB;
// ncls * nbins above 16,384 (40 x 4096) takes the path that adds into the global bins directly.
constexpr size_t kHistLdsBudget = 64 * 1024;
// Rounds of the wave-level combine below (0: one atomic per lane; an experiment build sets it
// with EXTRA=-DADAPTSEG_PSEUDO_PEEL=n, tools/bench_pseudo.py measures it)
#ifndef ADAPTSEG_PSEUDO_PEEL
#define ADAPTSEG_PSEUDO_PEEL 2
#endif
constexpr int kPeelRounds = ADAPTSEG_PSEUDO_PEEL;

inline int pseudo_grid(int64_t npix) {
  const int64_t b = ceil_div(npix, kPseudoPixPerBlock);
  return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

// A pixel counts when its class is one of the ncls and its confidence is a number >= 0
__device__ __forceinline__ bool pseudo_valid(int cls, float conf, int ncls) { return cls < ncls && conf >= 0.f; }

// bin = nbins-1 if conf >= 1, else (int)(conf * nbins): nbins is a power of two, so the fp32
// product is exact and below nbins for every conf < 1
__device__ __forceinline__ int conf_bin(float conf, int nbins) {
  return conf >= 1.f ? nbins - 1 : (int)(conf * (float)nbins);
}

// bins[key] += 1 for every lane with key >= 0, called by all 64 lanes of a wave together.  Real
// confidence maps put most pixels of a wave on ONE key (road, top bin), and equal addresses of
// one atomic wave-instruction are served one after the other; so up to kPeelRounds times the
// first pending lane's key is broadcast, the lanes that share it are counted with a ballot and
// that lane adds the count alone.  What is left (distinct keys, mostly) adds 1 per lane.
template <typename T>
__device__ __forceinline__ void wave_count(T *bins, int key) {
  const int lane = threadIdx.x & (kWave - 1);
  bool todo = key >= 0;
#pragma unroll
  for (int r = 0; r < kPeelRounds; ++r) {
    const unsigned long long pending = __ballot(todo);
    if (pending == 0ull) return;
    const int leader = __ffsll((long long)pending) - 1;
    const int k0 = __shfl(key, leader);
    const bool same = todo && key == k0;
    const unsigned long long group = __ballot(same);
    if (lane == leader) atomicAdd(&bins[k0], (T)__popcll(group));
    todo = todo && !same;
  }
  if (todo) atomicAdd(&bins[key], (T)1);
}

// hist[cls][bin] += 1 per valid pixel.  LDS: per-block bins, one 64-bit atomic per non-zero bin at
// the end (confusion_hist_kernel's structure); !LDS: the wave-combined adds go to hist directly.
// Every thread of a block runs the same number of rounds (wave_count is a wave-wide call).
template <bool LDS>
__global__ void __launch_bounds__(kPseudoThreads) conf_hist_kernel(int64_t npix, const uint8_t *__restrict__ pred,
                                                                   const float *__restrict__ conf, int ncls,
                                                                   int nbins, unsigned long long *hist) {
  extern __shared__ unsigned int bins[];
  const int nb = ncls * nbins;
  if (LDS) {
    for (int j = threadIdx.x; j < nb; j += blockDim.x) bins[j] = 0u;
    __syncthreads();
  }
  for (int64_t base = blockIdx.x * (int64_t)blockDim.x; base < npix; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = base + threadIdx.x;
    int key = -1;
    if (i < npix) {
      const int c = pred[i];
      const float p = conf[i];
      if (pseudo_valid(c, p, ncls)) key = c * nbins + conf_bin(p, nbins);
    }
    if (LDS) wave_count(bins, key);
    else wave_count(hist, key);
  }
  if (LDS) {
    __syncthreads();
    for (int j = threadIdx.x; j < nb; j += blockDim.x)
      if (bins[j]) atomicAdd(&hist[j], (unsigned long long)bins[j]);
  }
}

// One block per class.  T = sum_b hist[c][b]; K = ceil(portion * T) (fp64); b* = the largest bin
// whose suffix sum is >= K; thr[c] = min(b* / nbins, cap), or cap for an empty class.  Thread t
// owns the bins [t * per, (t + 1) * per); a suffix scan of the 256 chunk sums tells it what lies
// above its chunk, and the one thread whose chunk crosses K walks it from the top.
__global__ void __launch_bounds__(kPseudoThreads) pseudo_thresholds_kernel(const int64_t *__restrict__ hist,
                                                                           int nbins, double portion, float cap,
                                                                           float *__restrict__ thr) {
  __shared__ long long suffix[kPseudoThreads];
  const int c = blockIdx.x, t = threadIdx.x;
  const int per = nbins >= kPseudoThreads ? nbins / kPseudoThreads : 1;
  const int lo = t * per;
  const int64_t *h = hist + (int64_t)c * nbins;
  long long own = 0;
  if (lo < nbins)
    for (int j = 0; j < per; ++j) own += h[lo + j];
  suffix[t] = own;
  __syncthreads();
  for (int o = 1; o < kPseudoThreads; o <<= 1) {   // inclusive suffix sums (integers: exact)
    const long long add = t + o < kPseudoThreads ? suffix[t + o] : 0;
    __syncthreads();
    suffix[t] += add;
    __syncthreads();
  }
  const long long total = suffix[0];
  if (total == 0) {
    if (t == 0) thr[c] = cap;
    return;
  }
  const long long k = (long long)ceil(portion * (double)total);
  long long s = suffix[t] - own;   // the bins above this chunk
  if (lo < nbins && s < k && s + own >= k) {
    int b = lo + per - 1;
    for (; b > lo; --b) {
      s += h[b];
      if (s >= k) break;
    }
    thr[c] = fminf((float)b / (float)nbins, cap);
  }
}

// labels[i] = pred[i] where the pixel is valid and conf[i] >= thr[pred[i]], else ignore_label;
// kept[c] += the pixels kept for class c (per-block LDS counts, then one 64-bit atomic per class).
__global__ void __launch_bounds__(kPseudoThreads) pseudo_label_kernel(int64_t npix, const uint8_t *__restrict__ pred,
                                                                      const float *__restrict__ conf,
                                                                      const float *__restrict__ thr, int ncls,
                                                                      int ignore_label, int64_t *__restrict__ labels,
                                                                      unsigned long long *kept) {
  __shared__ float sthr[256];
  __shared__ unsigned int cnt[256];
  for (int j = threadIdx.x; j < ncls; j += blockDim.x) {
    sthr[j] = thr[j];
    cnt[j] = 0u;
  }
  __syncthreads();
  for (int64_t base = blockIdx.x * (int64_t)blockDim.x; base < npix; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = base + threadIdx.x;
    int key = -1;
    if (i < npix) {
      const int c = pred[i];
      const float p = conf[i];
      if (pseudo_valid(c, p, ncls) && p >= sthr[c]) key = c;
      labels[i] = key >= 0 ? key : ignore_label;
    }
    if (kept) wave_count(cnt, key);
  }
  if (kept) {
    __syncthreads();
    for (int j = threadIdx.x; j < ncls; j += blockDim.x)
      if (cnt[j]) atomicAdd(&kept[j], (unsigned long long)cnt[j]);
  }
}

}  // namespace

}  // namespace adaptseg

using namespace adaptseg;

extern "C" {

int adaptseg_conf_hist(int64_t npix, const uint8_t *pred, const float *conf, int ncls, int nbins, int64_t *hist,
                       adaptseg_stream_t stream) {
  AS_CHECK_ARG(npix >= 0, "conf_hist: bad npix %lld", (long long)npix);
  AS_CHECK_ARG(ncls >= 1 && ncls <= 256, "conf_hist: bad ncls %d (1..256)", ncls);
  AS_CHECK_ARG(nbins >= 2 && nbins <= 4096 && (nbins & (nbins - 1)) == 0,
               "conf_hist: bad nbins %d (a power of two in 2..4096)", nbins);
  AS_CHECK_ARG(npix == 0 || (pred && conf && hist), "conf_hist: bad args (null pointer)");
  if (npix == 0) return ADAPTSEG_OK;
  const size_t lds = (size_t)ncls * nbins * sizeof(unsigned int);
  unsigned long long *h = reinterpret_cast<unsigned long long *>(hist);
  if (lds <= kHistLdsBudget)
    conf_hist_kernel<true><<<pseudo_grid(npix), kPseudoThreads, lds, as_stream(stream)>>>(npix, pred, conf, ncls,
                                                                                         nbins, h);
  else
    conf_hist_kernel<false><<<pseudo_grid(npix), kPseudoThreads, 0, as_stream(stream)>>>(npix, pred, conf, ncls,
                                                                                        nbins, h);
  AS_CHECK_LAUNCH("conf_hist");
  return ADAPTSEG_OK;
}

int adaptseg_pseudo_thresholds(const int64_t *hist, int ncls, int nbins, double portion, float cap, float *thr,
                               adaptseg_stream_t stream) {
  AS_CHECK_ARG(ncls >= 1 && ncls <= 256, "pseudo_thresholds: bad ncls %d (1..256)", ncls);
  AS_CHECK_ARG(nbins >= 2 && nbins <= 4096 && (nbins & (nbins - 1)) == 0,
               "pseudo_thresholds: bad nbins %d (a power of two in 2..4096)", nbins);
  AS_CHECK_ARG(portion > 0.0 && portion <= 1.0, "pseudo_thresholds: bad portion %g (0 < portion <= 1)", portion);
  AS_CHECK_ARG(cap > 0.f && cap <= 1.f, "pseudo_thresholds: bad cap %g (0 < cap <= 1)", (double)cap);
  AS_CHECK_ARG(hist && thr, "pseudo_thresholds: bad args (null pointer)");
  pseudo_thresholds_kernel<<<ncls, kPseudoThreads, 0, as_stream(stream)>>>(hist, nbins, portion, cap, thr);
  AS_CHECK_LAUNCH("pseudo_thresholds");
  return ADAPTSEG_OK;
}

int adaptseg_pseudo_label(int64_t npix, const uint8_t *pred, const float *conf, const float *thr, int ncls,
                          int ignore_label, int64_t *labels, int64_t *kept, adaptseg_stream_t stream) {
  AS_CHECK_ARG(npix >= 0, "pseudo_label: bad npix %lld", (long long)npix);
  AS_CHECK_ARG(ncls >= 1 && ncls <= 256, "pseudo_label: bad ncls %d (1..256)", ncls);
  AS_CHECK_ARG(ignore_label >= 0 && ignore_label <= 255, "pseudo_label: bad ignore_label %d (0..255)", ignore_label);
  AS_CHECK_ARG(npix == 0 || (pred && conf && thr && labels), "pseudo_label: bad args (null pointer)");
  if (npix == 0) return ADAPTSEG_OK;
  pseudo_label_kernel<<<pseudo_grid(npix), kPseudoThreads, 0, as_stream(stream)>>>(
      npix, pred, conf, thr, ncls, ignore_label, labels, reinterpret_cast<unsigned long long *>(kept));
  AS_CHECK_LAUNCH("pseudo_label");
  return ADAPTSEG_OK;
}

}  // extern "C"
