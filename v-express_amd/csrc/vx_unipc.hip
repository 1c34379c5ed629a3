// Solver kernels declared in include/vexpress_hip_solvers.h: the UniPC update of the denoising loop
// (vx_overlap_unipc_step: the corrector of the step that ended at this sample and the predictor to the next one, written in
// the loop's variance-preserving frame).  float32 only: both element builds carry the same code.
#include "../../include/vexpress_hip_solvers.h"
#include "vx_common.h"
#include "vx_overlap.h"

extern "C" int vx_solvers_abi_version(void) { return VX_SOLVERS_ABI_VERSION; }

namespace {

__device__ __forceinline__ float4 scale4(float k, const float4 a) {
  return make_float4(k * a.x, k * a.y, k * a.z, k * a.w);
}

__device__ __forceinline__ float4 axpy4(const float4 acc, float k, const float4 a) {   // acc + k a
  return make_float4(acc.x + k * a.x, acc.y + k * a.y, acc.z + k * a.z, acc.w + k * a.w);
}

// One UniPC update per frame: the averaged v exactly as overlap_ddim_kernel sums it (mean_of_terms4), then
//   m = a_i x - s_i v;  xc = use_c ? q_s saved + q_m m + q_1 H[h1] + q_2 H[h2] + q_3 H[h3] : x
//   out = k_x xc + k_m m + k_1 H[h1] + k_2 H[h2];  saved = xc;  H[h_write] = m;  latents = out
// with H the three history slots (each laid out like the latents, `slot_sz` floats apart).  A slot < 0 is skipped and its
// buffer never read; without the corrector neither saved nor H[h3] is read.  h_write may be a slot just read (at third
// order the oldest one): every thread reads its own 16 bytes of each buffer before it writes them, and no thread touches
// another's.  One thread per (frame slot, channel, pixel quad): float4 loads and stores (hw % 4 == 0, 16-byte aligned
// rows).  The slot numbers and use_c are kernel arguments, so every branch is uniform over the grid.
__global__ void overlap_unipc_kernel(float* latents, int c, int total_frames, int hw, const float* preds, int f_window,
                                     const int32_t* terms, int max_terms, const int32_t* frame_ids, const float* count,
                                     int n_frames, float* history, size_t slot_sz, int h1, int h2, int h3, int h_write,
                                     float* saved, int use_c, float a_i, float s_i, float q_s, float q_m, float q_1,
                                     float q_2, float q_3, float k_x, float k_m, float k_1, float k_2) {
  const int hq = hw >> 2;
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;   // (frame slot, channel, pixel quad)
  long total = (long)n_frames * c * hq;
  if (idx >= total) return;
  int q = (int)(idx % hq);
  int ch = (int)((idx / hq) % c);
  int fs = (int)(idx / ((long)hq * c));
  int fr = frame_ids[fs];
  const float4 v = mean_of_terms4(preds, c, f_window, hw, terms, max_terms, fs, ch, 4 * q, count[fs]);
  const size_t off = ((size_t)ch * total_frames + fr) * hw + 4 * q;
  const float4 x = *reinterpret_cast<const float4*>(latents + off);
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  // every read first: the two slots both parts take, then what only the corrector takes
  const float4 H1 = h1 >= 0 ? *reinterpret_cast<const float4*>(history + (size_t)h1 * slot_sz + off) : zero;
  const float4 H2 = h2 >= 0 ? *reinterpret_cast<const float4*>(history + (size_t)h2 * slot_sz + off) : zero;
  float4 m;
  m.x = a_i * x.x - s_i * v.x;
  m.y = a_i * x.y - s_i * v.y;
  m.z = a_i * x.z - s_i * v.z;
  m.w = a_i * x.w - s_i * v.w;
  float4 xc = x;
  if (use_c) {
    const float4 sv = *reinterpret_cast<const float4*>(saved + off);
    xc = axpy4(scale4(q_s, sv), q_m, m);
    if (h1 >= 0) xc = axpy4(xc, q_1, H1);
    if (h2 >= 0) xc = axpy4(xc, q_2, H2);
    if (h3 >= 0) xc = axpy4(xc, q_3, *reinterpret_cast<const float4*>(history + (size_t)h3 * slot_sz + off));
  }
  float4 out = axpy4(scale4(k_x, xc), k_m, m);
  if (h1 >= 0) out = axpy4(out, k_1, H1);
  if (h2 >= 0) out = axpy4(out, k_2, H2);
  *reinterpret_cast<float4*>(saved + off) = xc;
  if (h_write >= 0) *reinterpret_cast<float4*>(history + (size_t)h_write * slot_sz + off) = m;
  *reinterpret_cast<float4*>(latents + off) = out;
}

bool slot_ok(int s) { return s >= -1 && s <= 2; }

}  // namespace

extern "C" int vx_overlap_unipc_step(float* latents, int c, int total_frames, int hw, const float* preds, int f_window,
                                     const int32_t* terms, int max_terms, const int32_t* frame_ids, const float* count,
                                     int n_frames, float* history, int h1, int h2, int h3, int h_write, float* saved,
                                     int use_c, float a_i, float s_i, float q_s, float q_m, float q_1, float q_2,
                                     float q_3, float k_x, float k_m, float k_1, float k_2, void* stream) {
  VX_REQUIRE(latents, "vx_overlap_unipc_step: latents is NULL");
  VX_REQUIRE(preds, "vx_overlap_unipc_step: preds is NULL");
  VX_REQUIRE(terms, "vx_overlap_unipc_step: terms is NULL");
  VX_REQUIRE(frame_ids, "vx_overlap_unipc_step: frame_ids is NULL");
  VX_REQUIRE(count, "vx_overlap_unipc_step: count is NULL");
  VX_REQUIRE(saved, "vx_overlap_unipc_step: saved is NULL");
  VX_REQUIRE(c > 0 && total_frames > 0 && hw > 0 && f_window > 0 && max_terms > 0 && n_frames > 0,
             "vx_overlap_unipc_step: c, total_frames, hw, f_window, max_terms and n_frames must be positive");
  VX_REQUIRE(hw % 4 == 0, "vx_overlap_unipc_step: hw = %d must be a multiple of 4", hw);
  VX_REQUIRE(slot_ok(h1), "vx_overlap_unipc_step: h1 = %d outside -1..2", h1);
  VX_REQUIRE(slot_ok(h2), "vx_overlap_unipc_step: h2 = %d outside -1..2", h2);
  VX_REQUIRE(slot_ok(h3), "vx_overlap_unipc_step: h3 = %d outside -1..2", h3);
  VX_REQUIRE(slot_ok(h_write), "vx_overlap_unipc_step: h_write = %d outside -1..2", h_write);
  VX_REQUIRE(history || (h1 < 0 && h2 < 0 && h3 < 0 && h_write < 0),
             "vx_overlap_unipc_step: history is NULL while a slot (h1, h2, h3, h_write) is >= 0");
  VX_REQUIRE(use_c == 0 || use_c == 1, "vx_overlap_unipc_step: use_c = %d outside 0..1", use_c);
  VX_REQUIRE(((uintptr_t)latents % 16) == 0 && ((uintptr_t)preds % 16) == 0 && ((uintptr_t)history % 16) == 0 &&
                 ((uintptr_t)saved % 16) == 0,
             "vx_overlap_unipc_step: latents, preds, history and saved must be 16-byte aligned");
  const long quads = (long)n_frames * c * (hw / 4);
  VX_REQUIRE(quads <= 0x7fffffffL * 256L, "vx_overlap_unipc_step: too many elements for one launch");
  hipLaunchKernelGGL(overlap_unipc_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     latents, c, total_frames, hw, preds, f_window, terms, max_terms, frame_ids, count, n_frames, history,
                     (size_t)c * total_frames * hw, h1, h2, h3, h_write, saved, use_c, a_i, s_i, q_s, q_m, q_1, q_2, q_3,
                     k_x, k_m, k_1, k_2);
  return vx_check_launch("vx_overlap_unipc_step");
}
