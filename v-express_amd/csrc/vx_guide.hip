// Guidance kernels declared in include/vexpress_hip_guidance.h: adaptive projected guidance (vx_guidance_apg).
// float32 only: both element builds carry the same code.
#include <math.h>

#include "../../include/vexpress_hip_guidance.h"
#include "vx_common.h"

#pragma clang fp contract(off)

extern "C" int vx_guidance_abi_version(void) { return VX_GUIDANCE_ABI_VERSION; }

// Adaptive projected guidance.  Per (window, frame slot) and per difference d_j = rows[j + 1] - rows[j] (two rows: c - u
// or c - m; three rows: m - u and c - m), over the frame's c * hw values with cv the last (fully conditional) row:
//   dbar_j = d_j + momentum * dbar_prev_j;  S_cc = sum cv^2,  S_dd_j = sum dbar_j^2,  S_dc_j = sum dbar_j cv
//   A_j = (s_j - 1) phi_j,  B_j = (s_j - 1) phi_j (1 - eta) k_j,  phi_j = min(1, r / sqrt(S_dd_j)),  k_j = S_dc_j / S_cc
//   g = (cv + A_0 dbar_0) - B_0 cv   [ ... + A_1 dbar_1) - B_1 cv ]
// Every product and sum of the float32 path is rounded on its own, never an fma: this file is compiled with floating-point
// contraction off (the pragma below; __fmul_rn / __fadd_rn are plain operators in the HIP headers and do not prevent it).
// Two launches over ONE partition: a block is (window, frame slot, chunk of APG_CHUNK pixels), a thread one pixel with its
// c channels (contiguous in `gathered`: one 16-byte load per row at c = 4; preds and the momentum buffers are
// channel-major, so a wave's stores of one channel are 256 contiguous bytes).  The partition depends on (f, hw) only.
// (1) apg_stats_kernel forms dbar (stored when momentum != 0), sums each thread's c values in channel order, then the
//     block: wave-64 shuffles, LDS across the waves in wave order; thread 0 writes the block's NS = 2 (ROWS - 1) + 1 sums
//     to its own place of the workspace.  No atomics.
// (2) apg_apply_kernel: thread 0 merges the frame's partials in ascending chunk order in double, forms A and B (each
//     rounded to float32 once), every thread writes g.
// Chunk size: 256 pixels = one per thread, so the per-thread chain is c adds (4: shorter than the 16 the error bound of
// the tests allows for) and the real window (16 frames of 4096 pixels) is 256 blocks, one per CU of the MI355X, in both
// launches; vx_guidance_rescale's 1024-pixel chunks give 64 blocks there, a quarter of the chip, with a 16-deep chain
// of dependent loads per thread.  Smaller chunks would only lengthen launch (2)'s serial merge.
constexpr int APG_CHUNK = 256;     // pixels per block
constexpr int APG_THREADS = 256;   // == APG_CHUNK: thread t of a block owns pixel chunk * APG_CHUNK + t
constexpr int APG_WAVES = APG_THREADS / 64;

// the ROWS values of one pixel's channel: C4 holds the pixel's four channels of every row in registers
template <int ROWS, bool C4>
struct ApgPixel {
  const float* p[ROWS];
  float v[ROWS][4];

  __device__ __forceinline__ ApgPixel(const float* gathered, const int32_t* unit_index, int wi, int li, int px, int shards,
                                      int c, int f_loc, int hw) {
    const int j = li / f_loc;
    const long unit_sz = (long)f_loc * hw * c;
    const long row = (long)(li - j * f_loc) * hw + px;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      p[r] = gathered + unit_index[(wi * ROWS + r) * shards + j] * unit_sz + row * c;
      if constexpr (C4) {
        const float4 t = *reinterpret_cast<const float4*>(p[r]);
        v[r][0] = t.x; v[r][1] = t.y; v[r][2] = t.z; v[r][3] = t.w;
      }
    }
  }

  __device__ __forceinline__ float at(int r, int ch) const {
    if constexpr (C4) return v[r][ch];
    else return p[r][ch];
  }
};

template <int ROWS, bool C4>
__global__ __launch_bounds__(APG_THREADS) void apg_stats_kernel(const float* __restrict__ gathered,
                                                                const int32_t* __restrict__ unit_index, int shards, int c,
                                                                int f, int f_loc, int hw, int chunks, long buf_elems,
                                                                float momentum, float* __restrict__ momentum_buf,
                                                                float* __restrict__ partials) {
  constexpr int ND = ROWS - 1, NS = 2 * ND + 1;
  __shared__ float lds[NS * APG_WAVES];
  const int chunk = blockIdx.x % chunks;
  const int li = (blockIdx.x / chunks) % f;
  const int wi = blockIdx.x / (chunks * f);
  const int px = chunk * APG_CHUNK + threadIdx.x;
  float s[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) s[i] = 0.f;
  if (px < hw) {
    const ApgPixel<ROWS, C4> rows(gathered, unit_index, wi, li, px, shards, c, f_loc, hw);
    const int cc = C4 ? 4 : c;
#pragma unroll
    for (int ch = 0; ch < cc; ++ch) {
      const float cv = rows.at(ROWS - 1, ch);
      s[0] = s[0] + cv * cv;
#pragma unroll
      for (int j = 0; j < ND; ++j) {
        float d = rows.at(j + 1, ch) - rows.at(j, ch);
        if (momentum != 0.f) {                               // uniform: a kernel argument
          float* m = momentum_buf + j * buf_elems + (((size_t)wi * c + ch) * f + li) * hw + px;
          d = d + momentum * *m;
          *m = d;
        }
        s[1 + 2 * j] = s[1 + 2 * j] + d * d;
        s[2 + 2 * j] = s[2 + 2 * j] + d * cv;
      }
    }
  }
  // the block's sums: a butterfly over the wave (every lane ends with the same bits), then the waves in wave order
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int i = 0; i < NS; ++i) s[i] = s[i] + __shfl_xor(s[i], off, 64);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0)
#pragma unroll
    for (int i = 0; i < NS; ++i) lds[wave * NS + i] = s[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    float* out = partials + (size_t)blockIdx.x * NS;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      float t = lds[i];
#pragma unroll
      for (int w = 1; w < APG_WAVES; ++w) t = t + lds[w * NS + i];
      out[i] = t;
    }
  }
}

template <int ROWS, bool C4>
__global__ __launch_bounds__(APG_THREADS) void apg_apply_kernel(const float* __restrict__ gathered,
                                                                const int32_t* __restrict__ unit_index, int shards, int c,
                                                                int f, int f_loc, int hw, int chunks, long buf_elems,
                                                                float scale0, float scale1, float eta, float norm_threshold,
                                                                float momentum, const float* __restrict__ momentum_buf,
                                                                const float* __restrict__ partials,
                                                                float* __restrict__ preds) {
  constexpr int ND = ROWS - 1, NS = 2 * ND + 1;
  __shared__ float coef[2 * ND];
  const int chunk = blockIdx.x % chunks;
  const int li = (blockIdx.x / chunks) % f;
  const int wi = blockIdx.x / (chunks * f);
  if (threadIdx.x == 0) {
    const float* p = partials + (size_t)(blockIdx.x - chunk) * NS;   // the frame's partials are consecutive blocks
    double S[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) S[i] = 0.0;
    for (int k = 0; k < chunks; ++k)                                 // ascending chunk order
#pragma unroll
      for (int i = 0; i < NS; ++i) S[i] += (double)p[(size_t)k * NS + i];
#pragma unroll
    for (int j = 0; j < ND; ++j) {
      const double sdd = S[1 + 2 * j], sdc = S[2 + 2 * j], scc = S[0];
      const double phi = (norm_threshold > 0.f && sdd > 0.0) ? fmin(1.0, (double)norm_threshold / sqrt(sdd)) : 1.0;
      const double k = scc > 0.0 ? sdc / scc : 0.0;
      const double a = ((double)(j == 0 ? scale0 : scale1) - 1.0) * phi;
      coef[2 * j] = (float)a;
      coef[2 * j + 1] = (float)(a * (1.0 - (double)eta) * k);
    }
  }
  __syncthreads();
  const int px = chunk * APG_CHUNK + threadIdx.x;
  if (px >= hw) return;
  const ApgPixel<ROWS, C4> rows(gathered, unit_index, wi, li, px, shards, c, f_loc, hw);
  const int cc = C4 ? 4 : c;
#pragma unroll
  for (int ch = 0; ch < cc; ++ch) {
    const size_t at = (((size_t)wi * c + ch) * f + li) * hw + px;
    const float cv = rows.at(ROWS - 1, ch);
    float g = cv;
#pragma unroll
    for (int j = 0; j < ND; ++j) {
      const float dbar = momentum != 0.f ? momentum_buf[j * buf_elems + at] : (rows.at(j + 1, ch) - rows.at(j, ch));
      g = (g + coef[2 * j] * dbar) - coef[2 * j + 1] * cv;
    }
    preds[at] = g;
  }
}

static inline int apg_chunks(int hw) { return (hw + APG_CHUNK - 1) / APG_CHUNK; }

extern "C" int64_t vx_guidance_apg_ws_floats(int n_windows, int rows, int f, int hw) {
  if (n_windows <= 0 || (rows != 2 && rows != 3) || f <= 0 || hw <= 0) return 0;
  return (int64_t)n_windows * f * apg_chunks(hw) * (2 * (rows - 1) + 1);
}

template <int ROWS, bool C4>
static int launch_apg(const float* gathered, const int32_t* unit_index, int n_windows, int shards, int c, int f, int hw,
                      float guidance, float audio_guidance, float eta, float norm_threshold, float momentum,
                      float* momentum_buf, float* workspace, float* preds, hipStream_t stream) {
  const int chunks = apg_chunks(hw);
  const dim3 grid((unsigned)((long)n_windows * f * chunks));
  const long buf_elems = (long)n_windows * c * f * hw;
  hipLaunchKernelGGL((apg_stats_kernel<ROWS, C4>), grid, dim3(APG_THREADS), 0, stream, gathered, unit_index, shards, c, f,
                     f / shards, hw, chunks, buf_elems, momentum, momentum_buf, workspace);
  int rc = vx_check_launch("vx_guidance_apg (statistics)");
  if (rc) return rc;
  hipLaunchKernelGGL((apg_apply_kernel<ROWS, C4>), grid, dim3(APG_THREADS), 0, stream, gathered, unit_index, shards, c, f,
                     f / shards, hw, chunks, buf_elems, guidance, audio_guidance, eta, norm_threshold, momentum,
                     (const float*)momentum_buf, (const float*)workspace, preds);
  return vx_check_launch("vx_guidance_apg");
}

extern "C" int vx_guidance_apg(const float* gathered, const int32_t* unit_index, int n_windows, int rows, int shards,
                               int c, int f, int hw, float guidance, float audio_guidance, float eta,
                               float norm_threshold, float momentum, float* momentum_buf, float* workspace,
                               int64_t ws_floats, float* preds, void* stream) {
  VX_REQUIRE(rows == 2 || rows == 3, "vx_guidance_apg: rows must be 2 or 3, got %d", rows);
  VX_REQUIRE(gathered && unit_index && workspace && preds && n_windows > 0 && shards > 0 && c > 0 && f > 0 && hw > 0 &&
                 f % shards == 0,
             "vx_guidance_apg: bad arguments");
  VX_REQUIRE(eta >= 0.f && eta <= 1.f, "vx_guidance_apg: eta must lie in [0, 1]");
  VX_REQUIRE(isfinite(norm_threshold) && norm_threshold >= 0.f,
             "vx_guidance_apg: norm_threshold must be finite and >= 0");
  VX_REQUIRE(fabsf(momentum) < 1.f, "vx_guidance_apg: momentum must satisfy |momentum| < 1");
  VX_REQUIRE(isfinite(guidance) && (rows == 2 || isfinite(audio_guidance)),
             "vx_guidance_apg: guidance / audio_guidance must be finite");
  VX_REQUIRE((momentum != 0.f) == (momentum_buf != nullptr),
             "vx_guidance_apg: momentum_buf must be given when momentum != 0 and NULL when momentum == 0");
  VX_REQUIRE((long)n_windows * f * apg_chunks(hw) <= 0x7fffffffL, "vx_guidance_apg: too many partials");
  VX_REQUIRE(ws_floats >= vx_guidance_apg_ws_floats(n_windows, rows, f, hw),
             "vx_guidance_apg: workspace too small (vx_guidance_apg_ws_floats)");
  const hipStream_t st = (hipStream_t)stream;
  // the 16-byte row loads need c = 4 and a 16-byte aligned buffer; the same sums in the same order either way
  const bool c4 = c == 4 && ((uintptr_t)gathered & 15) == 0;
#define VX_APG(ROWS, C4)                                                                                              \
  launch_apg<ROWS, C4>(gathered, unit_index, n_windows, shards, c, f, hw, guidance, audio_guidance, eta, norm_threshold, \
                       momentum, momentum_buf, workspace, preds, st)
  if (rows == 2) return c4 ? VX_APG(2, true) : VX_APG(2, false);
  return c4 ? VX_APG(3, true) : VX_APG(3, false);
#undef VX_APG
}
