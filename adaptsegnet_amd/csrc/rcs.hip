// Rare class sampling (RCS; Hoyer et al., DAFormer, CVPR 2022, section 3.2) on the decoded uint8 label files.
//   label_class_count   per image the number of pixels of every trainId: the statistics the sampler is built from
//   crop_class_count    per (sample, candidate window) the number of pixels of the sample's class in the label
//                       window adaptseg_gta5_preprocess_augment would return, WITHOUT resizing or materialising it
// The label window is separable, out[y][x] = lut[ids[ny[y]][nx[x]]], so a window's count of class c is
//   sum_sy sum_sx my[sy] * mx[sx] * [lut[ids[sy][sx]] == c]
// with mx / my the number of window columns / rows that read a source column / row.  One read of the label rows
// scores every candidate of a batch.  Integer atomics only: every count is exact and order-independent.
#include "common.hpp"
#include <algorithm>
#include <cmath>

namespace adaptseg {

namespace {

constexpr int kRcsThreads = 256;
constexpr int kRcsK = ADAPTSEG_RCS_MAX_CANDIDATES;   // candidate slots of the row tables (16: one 64-byte line)
static_assert(kRcsK == 16, "the row tables hold four 16-byte groups of candidates");

// ---- label_class_count -------------------------------------------------------------------------------------------
constexpr int kCountMaxBlocks = 1024;   // per batch; every block ends with at most num_classes 64-bit atomics

// bins[key] += 1 for every lane with key >= 0, called by all 64 lanes of a wave together: pseudo.hip's wave-level
// combine (two rounds: the first pending lane's key is broadcast, the lanes that share it are counted with a
// ballot and that lane adds the count alone; what is left adds 1 per lane).  A label map is mostly ONE class per
// wave, and equal addresses of one LDS atomic instruction are served one after the other.
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

// grid (blocks, images), 256 threads.  counts[img][c] += the image's pixels whose trainId is c (per-block LDS bins,
// one 64-bit atomic per non-zero bin).  VEC: hw % 16 == 0 and 16-byte aligned ids, 16 pixels per thread and sweep.
// Every thread of a block runs the same number of sweeps (wave_count is a wave-wide call).
template <bool VEC>
__global__ void __launch_bounds__(kRcsThreads) label_count_kernel(int hw, const uint8_t *__restrict__ ids,
                                                                  const int32_t *__restrict__ lut, int ncls,
                                                                  unsigned long long *counts) {
  __shared__ unsigned int bins[256];
  __shared__ int skey[256];   // id -> trainId, -1 where it counts nowhere
  {
    const int id = threadIdx.x;
    const int key = lut ? lut[id] : id;
    skey[id] = key >= 0 && key < ncls ? key : -1;
    bins[id] = 0u;
  }
  __syncthreads();
  const int img = blockIdx.y;
  ids += (int64_t)img * hw;
  if (VEC) {
    const int groups = hw >> 4;
    for (int g0 = blockIdx.x * kRcsThreads; g0 < groups; g0 += gridDim.x * kRcsThreads) {
      const int g = g0 + threadIdx.x;
      const bool have = g < groups;
      uint4 u = make_uint4(0u, 0u, 0u, 0u);
      if (have) u = *reinterpret_cast<const uint4 *>(ids + ((int64_t)g << 4));
      const uint32_t wd[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) wave_count(bins, have ? skey[(wd[q] >> (8 * j)) & 255u] : -1);
    }
  } else {
    for (int64_t i0 = (int64_t)blockIdx.x * kRcsThreads; i0 < hw; i0 += (int64_t)gridDim.x * kRcsThreads) {
      const int64_t i = i0 + threadIdx.x;
      wave_count(bins, i < hw ? skey[ids[i]] : -1);
    }
  }
  __syncthreads();
  const int c = threadIdx.x;
  if (c < ncls && bins[c]) atomicAdd(&counts[(int64_t)img * ncls + c], (unsigned long long)bins[c]);
}

// ---- crop_class_count --------------------------------------------------------------------------------------------
// Workspace, per call (every part 256-byte aligned):
//   hdr   int32  [n][8]              planes, ids that map to the class, column union [clo, chi), row hull [rlo, rhi)
//   idl   uint8  [n][256]            the ids whose trainId is the sample's class (the first hdr[1] entries)
//   mx    int32  [n][K][in_w]        column multiplicities (an intermediate of the prepare launch)
//   my    int32  [n][in_h][16]       row multiplicities, the 16 candidate slots of a row in one 64-byte line
//   win   uint32 [n][planes][T][16]  bit planes of mx: bit b of win[i][p][t][k] is bit p of mx[i][k][16 (t - 1) + b]
// The main launch reads a label row in 16-byte ALIGNED groups whatever the row's own alignment: group t of a row
// whose first byte sits a bytes past a 16-byte boundary holds the columns [16 t - a, 16 t - a + 16), which are the
// bits [16 - a, 32 - a) of window t.  Columns outside [0, in_w) have no bit set in any plane, so the bytes of a
// neighbouring row that an aligned group also holds count for nothing.
constexpr int kPrepThreads = 1024;   // 16 waves: wave k walks candidate k
constexpr int kPrepChunk = 8;        // samples per prepare launch (their parameters are kernel arguments)
constexpr int kCropMaxBlocks = 2048; // per batch, four label rows (one per wave) per block and sweep

struct RcsChunk {
  int p[kPrepChunk][kRcsK][5];   // sw, sh, ox, oy, mirror
};

struct RcsTables {
  int K, planes_cap, T;
  int *hdr;
  uint8_t *idl;
  int *mx, *my;
  uint32_t *win;
};

// A table entry the walks of this block added to with device-scope atomics: loaded at that scope too
__device__ __forceinline__ int rcs_load(const int *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

#pragma clang fp contract(off)
constexpr int kWalkRun = 32;   // positions per lane and pass of the walk

// The nearest-coordinate walk of augment_coeff_kernel (Pillow's sequential double accumulation, v = 0.5 * scale,
// then v += scale per position) over the scaled positions [lo, end) that fall inside the window, called by all 64
// lanes of a wave together; tab[s * stride] += how many of those positions read source index s (tab is zero on
// entry).  The accumulation is a chain of dependent additions, so every lane runs the SAME chain (one lane's
// cost) and lane j keeps the value it passes at position base + 32 j; from there the lane repeats the chain's
// next 32 additions, the same operands in the same order and so the same bits, and turns them into indices.  The
// indices never decrease: a lane counts a run in a register and adds it once.  [*first, *last] is the range of
// source indices read (first = -1: none), the same on every lane.
__device__ __forceinline__ void rcs_walk(int in, int out, int span, int off, bool flip, int *tab, int stride,
                                         int *first, int *last) {
  const int lane = threadIdx.x & (kWave - 1);
  const int lo = flip ? (out - off - span > 0 ? out - off - span : 0) : (off > 0 ? off : 0);
  const int end = flip ? (out - off < out ? out - off : out) : (off + span < out ? off + span : out);
  int f = -1, l = -1;
  if (lo < end) {
    const double scale = (double)in / (double)out;
    double v = 0.5 * scale;
    for (int o = 0; o < lo; ++o) v += scale;
    for (int base = lo; base < end; base += kWave * kWalkRun) {
      double mine = v;
      for (int j = 0; j < kWave; ++j) {
        if (lane == j) mine = v;
        if (base + kWalkRun * (j + 1) >= end) break;   // no lane starts later than this
#pragma unroll
        for (int i = 0; i < kWalkRun; ++i) v += scale;
      }
      int prev = -1, cnt = 0;
      const int o0 = base + kWalkRun * lane;
      for (int i = 0; i < kWalkRun && o0 + i < end; ++i) {
        int sidx = (int)mine;
        sidx = sidx < in - 1 ? sidx : in - 1;
        if (sidx != prev) {
          if (prev >= 0) atomicAdd(&tab[(int64_t)prev * stride], cnt);
          prev = sidx;
          cnt = 0;
        }
        ++cnt;
        if (o0 + i == lo) f = sidx;
        if (o0 + i == end - 1) l = sidx;
        mine += scale;
      }
      if (prev >= 0) atomicAdd(&tab[(int64_t)prev * stride], cnt);
    }
    for (int o = 32; o > 0; o >>= 1) {   // one lane holds each of them, the others -1
      const int fo = __shfl_xor(f, o), lo2 = __shfl_xor(l, o);
      f = fo > f ? fo : f;
      l = lo2 > l ? lo2 : l;
    }
  }
  *first = f;
  *last = l;
}
#pragma clang fp contract(on)

// grid (2, samples of the chunk), 1024 threads.  Block x = 0: the column tables of sample b (mx, its bit planes,
// the union of the candidates' column ranges) and the clear of counts[b][:]; block x = 1: the row table, the hull
// of the candidates' row ranges and the ids of the sample's class.
__global__ void __launch_bounds__(kPrepThreads) rcs_prepare_kernel(int first, int in_h, int in_w, int ch, int cw,
                                                                   RcsChunk c, RcsTables t,
                                                                   const int32_t *__restrict__ lut,
                                                                   const int32_t *__restrict__ classes,
                                                                   unsigned long long *counts) {
  __shared__ int s_first[kRcsK], s_last[kRcsK], s_max;
  const int s = blockIdx.y, b = first + s;
  const bool xs = blockIdx.x == 0;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & (kWave - 1);
  const int K = t.K;
  int *mx = t.mx + (int64_t)b * K * in_w;
  int *my = t.my + (int64_t)b * in_h * kRcsK;
  int *hdr = t.hdr + 8 * b;
  const int fill = xs ? K * in_w : in_h * kRcsK;
  for (int j = tid; j < fill; j += kPrepThreads) (xs ? mx : my)[j] = 0;
  if (xs && tid < K) counts[(int64_t)b * K + tid] = 0ull;
  __threadfence();   // the zeros are in memory before any lane adds to them
  __syncthreads();
  {
    int f = -1, l = -1;
    if (wave < K) {
      if (xs)
        rcs_walk(in_w, c.p[s][wave][0], cw, c.p[s][wave][2], c.p[s][wave][4] != 0, mx + (int64_t)wave * in_w, 1, &f,
                 &l);
      else
        rcs_walk(in_h, c.p[s][wave][1], ch, c.p[s][wave][3], false, my + wave, kRcsK, &f, &l);
    }
    if (lane == 0) {
      s_first[wave] = f;
      s_last[wave] = l;
    }
  }
  if (tid == 0) s_max = 0;
  __threadfence();
  __syncthreads();
  int lo = xs ? in_w : in_h, hi = 0;
#pragma unroll
  for (int k = 0; k < kRcsK; ++k) {
    if (s_first[k] >= 0) {
      lo = s_first[k] < lo ? s_first[k] : lo;
      hi = s_last[k] + 1 > hi ? s_last[k] + 1 : hi;
    }
  }
  if (!xs) {
    if (tid == 0) {
      hdr[4] = lo;
      hdr[5] = hi;
    }
    if (wave == 0) {
      const int cls = classes[b];
      uint8_t *idl = t.idl + 256 * b;
      int base = 0;
      for (int r = 0; r < 4; ++r) {
        const int id = r * kWave + lane;
        const bool hit = (lut ? lut[id] : id) == cls;
        const unsigned long long mask = __ballot(hit);
        if (hit) idl[base + __popcll(mask & ((1ull << lane) - 1ull))] = (uint8_t)id;
        base += __popcll(mask);
      }
      if (lane == 0) hdr[1] = base;
    }
    return;
  }
  // the largest column multiplicity of the sample (the walks added from every lane: read past the L1)
  int maxc = 0;
  for (int j = tid; j < K * in_w; j += kPrepThreads) {
    const int m = rcs_load(mx + j);
    maxc = m > maxc ? m : maxc;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const int mo = __shfl_xor(maxc, o);
    maxc = mo > maxc ? mo : maxc;
  }
  if (lane == 0 && maxc) atomicMax(&s_max, maxc);
  __syncthreads();
  maxc = s_max;
  int planes = 0;
  while ((maxc >> planes) != 0) ++planes;
  planes = planes < t.planes_cap ? planes : t.planes_cap;
  if (tid == 0) {
    hdr[0] = planes;
    hdr[2] = lo;
    hdr[3] = hi;
  }
  const int entries = t.T * kRcsK;
  for (int e = tid; e < entries; e += kPrepThreads) {
    const int tt = e >> 4, k = e & (kRcsK - 1);
    const int col0 = 16 * (tt - 1);
    for (int p = 0; p < planes; ++p) {
      uint32_t word = 0u;
      if (k < K) {
        for (int j = 0; j < 32; ++j) {
          const int col = col0 + j;
          if (col >= 0 && col < in_w) word |= (uint32_t)((rcs_load(mx + (int64_t)k * in_w + col) >> p) & 1) << j;
        }
      }
      t.win[(((int64_t)b * t.planes_cap + p) * t.T + tt) * kRcsK + k] = word;
    }
  }
}

// Four bytes of w against the byte v replicated in v4: bit j of the result = (byte j == v).  Exact: the sum
// (z & 0x7f..) + 0x7f.. sets a byte's top bit iff its low seven bits are non-zero and never carries across bytes;
// the multiply moves the four flags at bits 0, 8, 16, 24 to bits 24..27 (all partial products land on distinct bits).
__device__ __forceinline__ uint32_t eq4(uint32_t w, uint32_t v4) {
  const uint32_t z = w ^ v4;
  const uint32_t nz = ((z & 0x7f7f7f7fu) + 0x7f7f7f7fu) | z;
  const uint32_t e = (~nz & 0x80808080u) >> 7;
  return (e * 0x01020408u) >> 24 & 0xfu;
}

// grid (blocks, samples), 256 threads = 4 waves; a wave takes one label row per sweep, its lanes the row's aligned
// 16-byte groups.  KG: groups of four candidates (K <= 4 KG), the candidate loops unrolled over it so the
// accumulators stay in registers.  A lane's sum is part of one window's count, so it fits 32 bits (ch * cw < 2^31).
template <int KG>
__global__ void __launch_bounds__(kRcsThreads) crop_count_kernel(int n, int in_h, int in_w, RcsTables t,
                                                                 const uint8_t *__restrict__ ids,
                                                                 unsigned long long *counts) {
  constexpr int KK = 4 * KG;
  __shared__ unsigned int sums[KK];
  const int b = blockIdx.y;
  const int *hdr = t.hdr + 8 * b;
  const int planes = hdr[0], nids = hdr[1], clo = hdr[2], chi = hdr[3], rlo = hdr[4], rhi = hdr[5];
  if (planes == 0 || nids == 0 || clo >= chi || rlo >= rhi) return;   // counts[b][:] is already 0
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
  if (threadIdx.x < KK) sums[threadIdx.x] = 0u;
  __syncthreads();
  const uint8_t *idl = t.idl + 256 * b;
  const uint8_t *end = ids + (int64_t)n * in_h * in_w;
  uint32_t acc[KK];
#pragma unroll
  for (int k = 0; k < KK; ++k) acc[k] = 0u;
  for (int y = rlo + blockIdx.x * 4 + wave; y < rhi; y += gridDim.x * 4) {
    const int4 *mr = reinterpret_cast<const int4 *>(t.my + ((int64_t)b * in_h + y) * kRcsK);
    uint32_t myv[KK];
    uint32_t any = 0u;
#pragma unroll
    for (int g = 0; g < KG; ++g) {
      const int4 m = mr[g];
      myv[4 * g] = (uint32_t)m.x;
      myv[4 * g + 1] = (uint32_t)m.y;
      myv[4 * g + 2] = (uint32_t)m.z;
      myv[4 * g + 3] = (uint32_t)m.w;
      any |= (uint32_t)(m.x | m.y | m.z | m.w);
    }
    if (any == 0u) continue;   // a row no candidate reads
    const uint8_t *row = ids + ((int64_t)b * in_h + y) * in_w;
    const int a = (int)(reinterpret_cast<uintptr_t>(row) & 15u);
    const int sh = 16 - a;
    const int t1 = (chi + a + 15) >> 4;
    for (int tt = ((clo + a) >> 4) + lane; tt < t1; tt += kWave) {
      const uint8_t *p = row + (16 * tt - a);   // 16-byte aligned
      uint4 u;
      if (p >= ids && p + 16 <= end) {
        u = *reinterpret_cast<const uint4 *>(p);
      } else {   // the first or last group of the whole batch: byte by byte, 0 outside it
        uint32_t wd[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          wd[q] = 0u;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint8_t *pb = p + 4 * q + j;
            if (pb >= ids && pb < end) wd[q] |= (uint32_t)*pb << (8 * j);
          }
        }
        u = make_uint4(wd[0], wd[1], wd[2], wd[3]);
      }
      uint32_t bits = 0u;
      for (int q = 0; q < nids; ++q) {
        const uint32_t v4 = (uint32_t)idl[q] * 0x01010101u;
        bits |= eq4(u.x, v4) | eq4(u.y, v4) << 4 | eq4(u.z, v4) << 8 | eq4(u.w, v4) << 12;
      }
      if (bits == 0u) continue;
      uint32_t rc[KK];
#pragma unroll
      for (int k = 0; k < KK; ++k) rc[k] = 0u;
      for (int pl = 0; pl < planes; ++pl) {
        const uint4 *wp =
            reinterpret_cast<const uint4 *>(t.win + (((int64_t)b * t.planes_cap + pl) * t.T + tt) * kRcsK);
#pragma unroll
        for (int g = 0; g < KG; ++g) {
          const uint4 w = wp[g];
          rc[4 * g] += (uint32_t)__popc((w.x >> sh) & bits) << pl;
          rc[4 * g + 1] += (uint32_t)__popc((w.y >> sh) & bits) << pl;
          rc[4 * g + 2] += (uint32_t)__popc((w.z >> sh) & bits) << pl;
          rc[4 * g + 3] += (uint32_t)__popc((w.w >> sh) & bits) << pl;
        }
      }
#pragma unroll
      for (int k = 0; k < KK; ++k) acc[k] += myv[k] * rc[k];
    }
  }
#pragma unroll
  for (int k = 0; k < KK; ++k) {
    uint32_t v = acc[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0 && v) atomicAdd(&sums[k], v);
  }
  __syncthreads();
  if (threadIdx.x < t.K && sums[threadIdx.x])
    atomicAdd(&counts[(int64_t)b * t.K + threadIdx.x], (unsigned long long)sums[threadIdx.x]);
}

// adaptseg_gta5_preprocess_augment's limits (data.hip)
constexpr int kRcsMaxOffset = 1 << 20;
constexpr int kRcsMaxKsize = 64;

int rcs_ksize(int in_size, int out_size) {
  const double scale = (double)in_size / (double)out_size;
  const double support = 2.0 * (scale < 1.0 ? 1.0 : scale);
  return (int)std::ceil(support) * 2 + 1;
}

size_t rcs_a256(size_t b) { return (b + 255) / 256 * 256; }

struct RcsLayout {
  int planes_cap, T;
  size_t hdr, idl, mx, my, win, total;
};

// Host validation of a crop count's geometry and candidates (preprocess_augment's checks, with its limits), and
// the workspace layout.
int rcs_plan(int n, int in_h, int in_w, int ch, int cw, int K, const int32_t *params, RcsLayout *l) {
  AS_CHECK_ARG(n > 0 && in_h > 0 && in_w > 0 && ch > 0 && cw > 0, "crop_class_count: bad sizes");
  AS_CHECK_ARG(n <= 65535, "crop_class_count: bad n %d (at most 65535 samples per call)", n);
  AS_CHECK_ARG(K >= 1 && K <= kRcsK, "crop_class_count: bad K %d (1..%d candidates per sample)", K, kRcsK);
  AS_CHECK_ARG(ch < kRcsMaxOffset && cw < kRcsMaxOffset, "crop_class_count: crop size too large");
  AS_CHECK_ARG((int64_t)ch * cw < (1ll << 31), "crop_class_count: crop %d x %d (expected ch * cw < 2^31)", cw, ch);
  AS_CHECK_ARG((int64_t)in_h * in_w < (1ll << 31) && in_w < (1 << 24) && in_h < (1 << 24),
               "crop_class_count: labels %d x %d too large", in_w, in_h);
  AS_CHECK_ARG((int64_t)n * in_h * in_w < (1ll << 40), "crop_class_count: input too large");
  AS_CHECK_ARG(params, "crop_class_count: null params");
  int maxmult = 1;
  for (int b = 0; b < n; ++b) {
    for (int k = 0; k < K; ++k) {
      const int32_t *p = params + 5 * ((size_t)b * K + k);
      AS_CHECK_ARG(p[0] >= 1 && p[1] >= 1 && p[0] < kRcsMaxOffset && p[1] < kRcsMaxOffset,
                   "crop_class_count: bad scaled size %d x %d of sample %d, candidate %d", p[0], p[1], b, k);
      AS_CHECK_ARG(p[2] > -kRcsMaxOffset && p[2] < kRcsMaxOffset && p[3] > -kRcsMaxOffset && p[3] < kRcsMaxOffset,
                   "crop_class_count: bad offset (%d, %d) of sample %d, candidate %d", p[2], p[3], b, k);
      AS_CHECK_ARG(p[4] == 0 || p[4] == 1, "crop_class_count: bad mirror flag %d of sample %d, candidate %d", p[4], b,
                   k);
      AS_CHECK_ARG(rcs_ksize(in_w, p[0]) <= kRcsMaxKsize && rcs_ksize(in_h, p[1]) <= kRcsMaxKsize,
                   "crop_class_count: downscale factor above 15 not supported");
      // a source column is read by at most ceil(sw / in_w) window columns, + 2 for the walk's rounding at
      // either end of a run
      maxmult = std::max(maxmult, (int)ceil_div(p[0], in_w) + 2);
    }
  }
  l->planes_cap = 0;
  while ((maxmult >> l->planes_cap) != 0) ++l->planes_cap;
  l->T = (in_w + 30) / 16 + 1;   // groups t < (in_w + 15 + 15) / 16 are read
  size_t o = 0;
  l->hdr = o; o += rcs_a256((size_t)n * 8 * 4);
  l->idl = o; o += rcs_a256((size_t)n * 256);
  l->mx = o; o += rcs_a256((size_t)n * K * in_w * 4);
  l->my = o; o += rcs_a256((size_t)n * in_h * kRcsK * 4);
  l->win = o; o += rcs_a256((size_t)n * l->planes_cap * l->T * kRcsK * 4);
  l->total = o;
  return ADAPTSEG_OK;
}

}  // namespace

}  // namespace adaptseg

using namespace adaptseg;

extern "C" {

int adaptseg_label_class_count(int n, int h, int w, const uint8_t *ids, const int32_t *lut, int num_classes,
                               int64_t *counts, adaptseg_stream_t stream) {
  AS_CHECK_ARG(n >= 1 && h >= 1 && w >= 1, "label_class_count: bad shape n %d, h %d, w %d", n, h, w);
  AS_CHECK_ARG(n <= 65535, "label_class_count: bad n %d (at most 65535 images per call)", n);
  AS_CHECK_ARG((int64_t)h * w < (1ll << 31), "label_class_count: %d x %d pixels per image (expected h * w < 2^31)", h,
               w);
  AS_CHECK_ARG(num_classes >= 1 && num_classes <= 255, "label_class_count: bad num_classes %d (1..255)", num_classes);
  AS_CHECK_ARG(ids && counts, "label_class_count: bad args (null pointer)");
  const int hw = h * w;
  hipStream_t s = as_stream(stream);
  // the kernel adds into counts: cleared here, on the stream, first
  if (hipMemsetAsync(counts, 0, (size_t)n * num_classes * sizeof(int64_t), s) != hipSuccess) {
    set_error("label_class_count: clearing the counts failed: %s", hipGetErrorString(hipGetLastError()));
    return ADAPTSEG_ERR_HIP;
  }
  const bool vec = hw % 16 == 0 && (reinterpret_cast<uintptr_t>(ids) & 15u) == 0;
  const int64_t want = ceil_div(hw, (int64_t)kRcsThreads * (vec ? 16 : 1));
  const int64_t cap = std::max(1, kCountMaxBlocks / n);
  const dim3 grid((unsigned)std::min(want, cap), (unsigned)n);
  unsigned long long *c = reinterpret_cast<unsigned long long *>(counts);
  if (vec) label_count_kernel<true><<<grid, kRcsThreads, 0, s>>>(hw, ids, lut, num_classes, c);
  else label_count_kernel<false><<<grid, kRcsThreads, 0, s>>>(hw, ids, lut, num_classes, c);
  AS_CHECK_LAUNCH("label_class_count");
  return ADAPTSEG_OK;
}

int adaptseg_crop_class_count_workspace_size(int n, int in_h, int in_w, int ch, int cw, int K, const int32_t *params,
                                             size_t *bytes) {
  AS_CHECK_ARG(bytes, "crop_class_count_workspace_size: null bytes");
  RcsLayout l;
  const int st = rcs_plan(n, in_h, in_w, ch, cw, K, params, &l);
  if (st != ADAPTSEG_OK) return st;
  *bytes = l.total;
  return ADAPTSEG_OK;
}

int adaptseg_crop_class_count(int n, int in_h, int in_w, int ch, int cw, int K, const uint8_t *ids,
                              const int32_t *lut, const int32_t *classes, const int32_t *params, int64_t *counts,
                              void *workspace, size_t ws_bytes, adaptseg_stream_t stream) {
  RcsLayout l;
  const int st = rcs_plan(n, in_h, in_w, ch, cw, K, params, &l);
  if (st != ADAPTSEG_OK) return st;
  AS_CHECK_ARG(ids && classes && counts, "crop_class_count: bad args (null pointer)");
  if (!workspace || ws_bytes < l.total) {
    set_error("crop_class_count: workspace %zu < required %zu", ws_bytes, l.total);
    return ADAPTSEG_ERR_WORKSPACE;
  }
  AS_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15u) == 0, "crop_class_count: workspace not 16-byte aligned");
  char *base = reinterpret_cast<char *>(workspace);
  RcsTables t;
  t.K = K;
  t.planes_cap = l.planes_cap;
  t.T = l.T;
  t.hdr = reinterpret_cast<int *>(base + l.hdr);
  t.idl = reinterpret_cast<uint8_t *>(base + l.idl);
  t.mx = reinterpret_cast<int *>(base + l.mx);
  t.my = reinterpret_cast<int *>(base + l.my);
  t.win = reinterpret_cast<uint32_t *>(base + l.win);
  hipStream_t s = as_stream(stream);
  unsigned long long *c = reinterpret_cast<unsigned long long *>(counts);
  // the prepare launch clears counts; the main launch adds into it
  for (int first = 0; first < n; first += kPrepChunk) {
    const int m = std::min(kPrepChunk, n - first);
    RcsChunk ck = {};
    for (int i = 0; i < m; ++i)
      for (int k = 0; k < K; ++k)
        for (int j = 0; j < 5; ++j) ck.p[i][k][j] = params[5 * ((size_t)(first + i) * K + k) + j];
    rcs_prepare_kernel<<<dim3(2u, (unsigned)m), kPrepThreads, 0, s>>>(first, in_h, in_w, ch, cw, ck, t, lut, classes,
                                                                      c);
    AS_CHECK_LAUNCH("crop_class_count prepare");
  }
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div(in_h, 4), std::max(1, kCropMaxBlocks / n)), (unsigned)n);
  switch ((K + 3) / 4) {
    case 1: crop_count_kernel<1><<<grid, kRcsThreads, 0, s>>>(n, in_h, in_w, t, ids, c); break;
    case 2: crop_count_kernel<2><<<grid, kRcsThreads, 0, s>>>(n, in_h, in_w, t, ids, c); break;
    case 3: crop_count_kernel<3><<<grid, kRcsThreads, 0, s>>>(n, in_h, in_w, t, ids, c); break;
    default: crop_count_kernel<4><<<grid, kRcsThreads, 0, s>>>(n, in_h, in_w, t, ids, c); break;
  }
  AS_CHECK_LAUNCH("crop_class_count");
  return ADAPTSEG_OK;
}

}  // extern "C"
