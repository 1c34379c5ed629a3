// Latent resize declared in include/vexpress_hip_resize.h: float32 planes [h, w] -> [h2, w2] from per-axis tap tables
// (bilinear: 2 taps, bicubic: 4), once per clip between the two passes of hi-res sampling.  float32 only: both element
// builds carry the same code.
// One thread per (plane, output row, quad of output columns); a wave's stores of one row are contiguous.  Every output is
// written by exactly one thread: no atomics, no workspace, no LDS.
#include <stdint.h>

#include "../../include/vexpress_hip_resize.h"
#include "vx_common.h"

extern "C" int vx_resize_abi_version(void) { return VX_RESIZE_ABI_VERSION; }

namespace {

// The summation order of the header: rows outer, columns inner, taps ascending, the first term of each sum initialises
// it.  Contraction is off, so every product and every sum is one float32 rounding.
template <int TAPS>
__global__ __launch_bounds__(256) void latent_resize_kernel(const float* __restrict__ src, int h, int w,
                                                            float* __restrict__ dst, int h2, int w2,
                                                            const int32_t* __restrict__ iy, const float* __restrict__ wy,
                                                            const int32_t* __restrict__ ix, const float* __restrict__ wx,
                                                            long total) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;   // (plane, output row, column quad)
  if (idx >= total) return;
  const int quads = (w2 + 3) >> 2;
  const int q = (int)(idx % quads);
  const int y = (int)((idx / quads) % h2);
  const long p = idx / ((long)quads * h2);
  const float* sp = src + (size_t)p * h * w;
  const float* rows[TAPS];
  float wrow[TAPS];
#pragma unroll
  for (int a = 0; a < TAPS; ++a) {
    rows[a] = sp + (size_t)min(max(iy[y * TAPS + a], 0), h - 1) * w;
    wrow[a] = wy[y * TAPS + a];
  }
  const int n = min(4, w2 - 4 * q);
  float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k >= n) break;
    const int x = 4 * q + k;
    int col[TAPS];
    float wcol[TAPS];
#pragma unroll
    for (int b = 0; b < TAPS; ++b) {
      col[b] = min(max(ix[x * TAPS + b], 0), w - 1);
      wcol[b] = wx[x * TAPS + b];
    }
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < TAPS; ++a) {
      float r = wcol[0] * rows[a][col[0]];
#pragma unroll
      for (int b = 1; b < TAPS; ++b) r = r + wcol[b] * rows[a][col[b]];
      const float t = wrow[a] * r;
      acc = a == 0 ? t : acc + t;
    }
    v[k] = acc;
  }
  float* out = dst + ((size_t)p * h2 + y) * w2 + 4 * q;
  if (n == 4 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0) {
    *reinterpret_cast<float4*>(out) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int k = 0; k < n; ++k) out[k] = v[k];
  }
}

}  // namespace

extern "C" int vx_latent_resize(const float* src, int planes, int h, int w, float* dst, int h2, int w2,
                                const int32_t* iy, const float* wy, const int32_t* ix, const float* wx, int taps,
                                void* stream) {
  VX_REQUIRE(src && dst, "vx_latent_resize: src / dst must be given");
  VX_REQUIRE(src != dst, "vx_latent_resize: dst must not be src");
  VX_REQUIRE(iy && wy && ix && wx, "vx_latent_resize: the tap tables iy / wy / ix / wx must be given");
  VX_REQUIRE(taps == 2 || taps == 4, "vx_latent_resize: taps must be 2 (bilinear) or 4 (bicubic), got %d", taps);
  VX_REQUIRE(planes > 0 && h > 0 && w > 0 && h2 > 0 && w2 > 0,
             "vx_latent_resize: planes, h, w, h2, w2 must be positive, got %d, %d, %d, %d, %d", planes, h, w, h2, w2);
  VX_REQUIRE((long)h2 * taps <= 0x7fffffffL && (long)w2 * taps <= 0x7fffffffL,
             "vx_latent_resize: h2 * taps / w2 * taps is too large for the tables' int index");
  const long total = (long)planes * h2 * ((w2 + 3) >> 2);
  VX_REQUIRE((total + 255) / 256 <= 0x7fffffffL, "vx_latent_resize: planes * h2 * w2 is too large for one launch");
  const dim3 grid((unsigned)((total + 255) / 256));
  const hipStream_t st = (hipStream_t)stream;
  if (taps == 2)
    hipLaunchKernelGGL(latent_resize_kernel<2>, grid, dim3(256), 0, st, src, h, w, dst, h2, w2, iy, wy, ix, wx, total);
  else
    hipLaunchKernelGGL(latent_resize_kernel<4>, grid, dim3(256), 0, st, src, h, w, dst, h2, w2, iy, wy, ix, wx, total);
  return vx_check_launch("vx_latent_resize");
}
