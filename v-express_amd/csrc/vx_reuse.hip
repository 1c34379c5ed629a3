// Guidance-reuse kernels declared in include/vexpress_hip_reuse.h: the combine of a refresh step, which also stores the
// differences of consecutive rows (vx_combine_units_keep), and the combine of a reuse step, which adds stored differences
// to the conditional row (vx_combine_reused).  float32 only: both element builds carry the same code.
// Both use combine_units_kernel's partition (vx_elem.hip): one thread per (window, frame slot, pixel), the c channels of
// that pixel contiguous in `gathered`; preds and the difference slots are channel-major, so a wave's stores of one
// channel are 256 contiguous bytes.  Every element is read and written by exactly one thread: no atomics, no workspace.
#include <math.h>

#include "../../include/vexpress_hip_reuse.h"
#include "vx_common.h"
#include "vx_guidance_mix.h"

extern "C" int vx_reuse_abi_version(void) { return VX_REUSE_ABI_VERSION; }

namespace {

inline dim3 grid1d(long n, int bs = 256) { return dim3((unsigned)((n + bs - 1) / bs)); }

// where thread `idx` of the partition works: (window, frame slot, pixel), the shard that holds the frame slot and the
// offset of the pixel's channels inside a unit
struct UnitPixel {
  int wi, li, px, j;
  long row;

  __device__ __forceinline__ UnitPixel(long idx, int f, int f_loc, int hw) {
    px = (int)(idx % hw);
    li = (int)((idx / hw) % f);
    wi = (int)(idx / ((long)hw * f));
    j = li / f_loc;
    row = (long)(li - j * f_loc) * hw + px;
  }
};

// preds: the prologue and the channel loop of combine_units_kernel<ROWS> (vx_elem.hip) as they stand there, over the same
// guided_value<ROWS>, under the same contraction rule (the compiler's default) - the stores of the differences are a
// loop of their own after it, so that the compiler sees the loop it sees there and forms the same multiply-adds.
// diffs[k]: rows[k + 1] - rows[k] (the rows are in cache from the first loop)
template <int ROWS>
__global__ __launch_bounds__(256) void combine_units_keep_kernel(const float* __restrict__ gathered,
                                                                 const int32_t* __restrict__ unit_index, int n_windows,
                                                                 int shards, int c, int f, int f_loc, int hw,
                                                                 float guidance, float audio, size_t slot_elems,
                                                                 float* __restrict__ diffs, float* __restrict__ preds) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;   // (window, li, pixel)
  long total = (long)n_windows * f * hw;
  if (idx >= total) return;
  int px = (int)(idx % hw);
  int li = (int)((idx / hw) % f);
  int wi = (int)(idx / ((long)hw * f));
  int j = li / f_loc;
  long row = (long)(li - j * f_loc) * hw + px;
  long unit_sz = (long)f_loc * hw * c;
  const float* rows[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) rows[r] = gathered + unit_index[(wi * ROWS + r) * shards + j] * unit_sz + row * c;
  for (int ch = 0; ch < c; ++ch)
    preds[(((size_t)wi * c + ch) * f + li) * hw + px] = guided_value<ROWS>(rows, ch, guidance, audio);
  for (int ch = 0; ch < c; ++ch)
#pragma unroll
    for (int k = 0; k + 1 < ROWS; ++k)
      diffs[k * slot_elems + (((size_t)wi * c + ch) * f + li) * hw + px] = rows[k + 1][ch] - rows[k][ch];
}

// p = c + a1 L1 [+ b1 P1] [+ a2 L2 [+ b2 P2]], every product and every sum rounded on its own
template <int ND, bool PREV>
__global__ __launch_bounds__(256) void combine_reused_kernel(const float* __restrict__ gathered,
                                                             const int32_t* __restrict__ unit_index, int n_windows,
                                                             int shards, int c, int f, int f_loc, int hw,
                                                             size_t slot_elems, const float* __restrict__ last,
                                                             const float* __restrict__ prev, float a1, float b1, float a2,
                                                             float b2, float* __restrict__ preds) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)n_windows * f * hw) return;
  const UnitPixel at(idx, f, f_loc, hw);
  const float* cnd = gathered + unit_index[at.wi * shards + at.j] * ((long)f_loc * hw * c) + at.row * c;
  for (int ch = 0; ch < c; ++ch) {
    const size_t o = (((size_t)at.wi * c + ch) * f + at.li) * hw + at.px;
    float p = cnd[ch] + a1 * last[o];
    if constexpr (PREV) p = p + b1 * prev[o];
    if constexpr (ND == 2) {
      p = p + a2 * last[slot_elems + o];
      if constexpr (PREV) p = p + b2 * prev[slot_elems + o];
    }
    preds[o] = p;
  }
}

}  // namespace

extern "C" int vx_combine_units_keep(const float* gathered, const int32_t* unit_index, int n_windows, int rows,
                                     int shards, int c, int f, int hw, float guidance, float audio_guidance,
                                     float* diffs, float* preds, void* stream) {
  VX_REQUIRE(rows == 2 || rows == 3, "vx_combine_units_keep: rows must be 2 or 3, got %d", rows);
  VX_REQUIRE(gathered && unit_index, "vx_combine_units_keep: gathered / unit_index must be given");
  VX_REQUIRE(diffs, "vx_combine_units_keep: diffs must be given");
  VX_REQUIRE(preds, "vx_combine_units_keep: preds must be given");
  VX_REQUIRE(n_windows > 0 && shards > 0 && c > 0 && f > 0 && hw > 0 && f % shards == 0,
             "vx_combine_units_keep: n_windows, shards, c, f, hw must be positive and f a multiple of shards");
  VX_REQUIRE(isfinite(guidance) && (rows == 2 || isfinite(audio_guidance)),
             "vx_combine_units_keep: guidance / audio_guidance must be finite");
  const long threads = (long)n_windows * f * hw;
  VX_REQUIRE((threads + 255) / 256 <= 0x7fffffffL, "vx_combine_units_keep: n_windows * f * hw is too large for one launch");
  const size_t slot = (size_t)threads * c;
  const hipStream_t st = (hipStream_t)stream;
  if (rows == 2)
    hipLaunchKernelGGL(combine_units_keep_kernel<2>, grid1d(threads), dim3(256), 0, st, gathered, unit_index, n_windows,
                       shards, c, f, f / shards, hw, guidance, 0.f, slot, diffs, preds);
  else
    hipLaunchKernelGGL(combine_units_keep_kernel<3>, grid1d(threads), dim3(256), 0, st, gathered, unit_index, n_windows,
                       shards, c, f, f / shards, hw, guidance, audio_guidance, slot, diffs, preds);
  return vx_check_launch("vx_combine_units_keep");
}

extern "C" int vx_combine_reused(const float* gathered, const int32_t* unit_index, int n_windows, int n_diffs,
                                 int shards, int c, int f, int hw, const float* last, const float* prev, float a1,
                                 float b1, float a2, float b2, float* preds, void* stream) {
  VX_REQUIRE(n_diffs == 1 || n_diffs == 2, "vx_combine_reused: n_diffs must be 1 or 2, got %d", n_diffs);
  VX_REQUIRE(gathered && unit_index, "vx_combine_reused: gathered / unit_index must be given");
  VX_REQUIRE(last, "vx_combine_reused: last must be given");
  VX_REQUIRE(preds, "vx_combine_reused: preds must be given");
  VX_REQUIRE(n_windows > 0 && shards > 0 && c > 0 && f > 0 && hw > 0 && f % shards == 0,
             "vx_combine_reused: n_windows, shards, c, f, hw must be positive and f a multiple of shards");
  VX_REQUIRE(isfinite(a1) && isfinite(b1) && isfinite(a2) && isfinite(b2),
             "vx_combine_reused: a1, b1, a2, b2 must be finite");
  VX_REQUIRE(n_diffs == 2 || (a2 == 0.f && b2 == 0.f), "vx_combine_reused: a2 and b2 must be 0 when n_diffs is 1");
  VX_REQUIRE((b1 != 0.f || b2 != 0.f) == (prev != nullptr),
             "vx_combine_reused: prev must be given when b1 or b2 is not 0 and NULL when both are 0");
  const long threads = (long)n_windows * f * hw;
  VX_REQUIRE((threads + 255) / 256 <= 0x7fffffffL, "vx_combine_reused: n_windows * f * hw is too large for one launch");
  const size_t slot = (size_t)threads * c;
  const hipStream_t st = (hipStream_t)stream;
#define VX_REUSED(ND, PREV)                                                                                              \
  hipLaunchKernelGGL((combine_reused_kernel<ND, PREV>), grid1d(threads), dim3(256), 0, st, gathered, unit_index,         \
                     n_windows, shards, c, f, f / shards, hw, slot, last, prev, a1, b1, a2, b2, preds)
  if (n_diffs == 1) {
    if (prev) VX_REUSED(1, true); else VX_REUSED(1, false);
  } else {
    if (prev) VX_REUSED(2, true); else VX_REUSED(2, false);
  }
#undef VX_REUSED
  return vx_check_launch("vx_combine_reused");
}
