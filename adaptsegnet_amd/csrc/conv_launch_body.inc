// Body shared by conv_launch_{fwd,dgrad,wgrad}.hip: each defines LAUNCH_NAME / LAUNCH_MODE
// and includes conv_kernels.hpp, then this file, so every product compiles in parallel.

namespace adaptseg {

#define AS_FAST(BM_, BN_, WM_, WN_, FBK_, S2_, AE_, BE_) \
  launch_k(igemm_fast_kernel<MODE, BM_, BN_, WM_, WN_, FBK_, S2_, AE_, BE_, MINB_>, grid, block, s, pl.p)

#define AS_LAUNCH(BM_, BN_, WM_, WN_, FBK_)                                                  \
  do {                                                                                       \
    if (pl.family == Family::Fast) {                                                         \
      const int v = (pl.s2 ? 4 : 0) | (pl.ae ? 2 : 0) | (pl.be ? 1 : 0);                     \
      switch (v) {                                                                           \
        case 0: AS_FAST(BM_, BN_, WM_, WN_, FBK_, false, false, false); break;              \
        case 1: AS_FAST(BM_, BN_, WM_, WN_, FBK_, false, false, true); break;               \
        case 2: AS_FAST(BM_, BN_, WM_, WN_, FBK_, false, true, false); break;               \
        case 3: AS_FAST(BM_, BN_, WM_, WN_, FBK_, false, true, true); break;                \
        case 4: if constexpr (MODE == MODE_DGRAD) AS_FAST(BM_, BN_, WM_, WN_, FBK_, true, false, false); break; \
        case 5: if constexpr (MODE == MODE_DGRAD) AS_FAST(BM_, BN_, WM_, WN_, FBK_, true, false, true); break;  \
        default: break;                                                                      \
      }                                                                                      \
    } else if (pl.va && pl.vb) {                                                             \
      launch_k(igemm_kernel<MODE, BM_, BN_, WM_, WN_, true, true>, grid, block, s, pl.p);       \
    } else if (pl.va) {                                                                      \
      launch_k(igemm_kernel<MODE, BM_, BN_, WM_, WN_, true, false>, grid, block, s, pl.p);      \
    } else if (pl.vb) {                                                                      \
      launch_k(igemm_kernel<MODE, BM_, BN_, WM_, WN_, false, true>, grid, block, s, pl.p);      \
    } else {                                                                                 \
      launch_k(igemm_kernel<MODE, BM_, BN_, WM_, WN_, false, false>, grid, block, s, pl.p);     \
    }                                                                                        \
  } while (0)

template <int MODE>
static hipError_t launch_cfg(const Plan &pl, hipStream_t s) {
  constexpr int MINB_ = 1;
  dim3 grid(pl.tiles, pl.p.splits, pl.s2 ? 4 : 1), block(pl.tile.threads);
  switch (pl.cfg) {
    case 0:
      // stride-1 vector data gradients (the 3x3 ones): the min-blocks-2 build (157 VGPRs, the
      // accumulators out of AGPRs, no SGPR spills; +0.3 % c2, +-0 c3 over min-blocks 1)
      if constexpr (MODE == MODE_DGRAD) {
        if (pl.family == Family::Fast && !pl.s2 && !pl.ae && !pl.be) {
          launch_k(igemm_fast_kernel<MODE, 128, 128, 2, 2, 32, false, false, false, 2>, grid, block, s, pl.p);
          break;
        }
      }
      AS_LAUNCH(128, 128, 2, 2, 32);
      break;
    case 1: AS_LAUNCH(256, 32, 4, 1, 32); break;
    // 32x256 / 64x256 / 64x64 serve only the weight gradient (M' = Cout <= 64): not
    // instantiated for the other products (their per-element variants would need scratch)
    case 2: if constexpr (MODE == MODE_WGRAD) { AS_LAUNCH(32, 256, 1, 4, 32); break; } else return hipErrorInvalidValue;
    case 3: if constexpr (MODE == MODE_WGRAD) { AS_LAUNCH(64, 256, 1, 4, 32); break; } else return hipErrorInvalidValue;
    case 4: AS_LAUNCH(256, 64, 4, 1, 16); break;
    case 5: if constexpr (MODE == MODE_WGRAD) { AS_LAUNCH(64, 64, 2, 2, 32); break; } else return hipErrorInvalidValue;
    case 6: AS_LAUNCH(128, 128, 2, 2, 16); break;
    case 7: AS_LAUNCH(256, 128, 4, 2, 32); break;
    default:
      // cfg 8: occupancy-3 build of the BK-16 tile (vector FAST operands only)
      if (pl.family != Family::Fast || pl.s2 || pl.ae || pl.be) return hipErrorInvalidValue;
      launch_k(igemm_fast_kernel<MODE, 128, 128, 2, 2, 16, false, false, false, 3>, grid, block, s, pl.p);
      break;
  }
  return hipGetLastError();
}

hipError_t LAUNCH_NAME(const Plan &pl, hipStream_t s) { return launch_cfg<LAUNCH_MODE>(pl, s); }

}  // namespace adaptseg
